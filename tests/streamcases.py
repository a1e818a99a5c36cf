"""Inputs and helpers for tests of stream order: calls queued on a stream BEHIND pending work that is still to write their inputs ("Streams").
Test infrastructure; numpy only, no device. tests/test_stream_order_host.py checks its premises on the host; the GPU tests that queue the calls are still
to be written on top of it.

Two variants, A and B, of one batch: the same CSR offsets and edge types, so that B can be written over A in place on the device, and nothing else in
common -- B's control points are A's reflected through the centre of the glyph's bounds (a half turn: windings keep their sign), its colours have red and
blue exchanged, its transforms frame the reflected glyph with another pixel range and a shift of a fraction of a texel, its boxes are those of another glyph,
its byte rectangles lie elsewhere in the atlas. A kernel that reads any input too early therefore writes other bytes for EVERY glyph
(tests/test_stream_order_host.py asserts that for the oracle's tiles; a GPU test asserts it for every output it compares: equal_glyphs)."""
import functools

import numpy as np

W, H = 24, 17                                      # the uniform tile: nine 8 x 8 tiles per glyph, both sides off the tile grid
PX_A, PX_B = 2., 3.                                # pixel ranges of the two variants
SHIFT_B = (.37, -.21)                              # B's transforms are moved by this many texels
ATLAS_FILL, ATLAS_PAD = 0xA5, 8


def mirrored(shape):
    """Variant B of a FlatShape: same offsets and types; points reflected through the centre of the bounds, red and blue exchanged."""
    from msdfgen_amd.shape import FlatShape
    l, b, r, t = shape.bounds()
    pts = np.array(shape.points, np.float64)
    for k in range(4):
        used = shape.types >= max(k, 1)                                    # (the control points FlatShape.bounds() counts)
        pts[used, 2*k] = (l+r)-pts[used, 2*k]
        pts[used, 2*k+1] = (b+t)-pts[used, 2*k+1]
    c = np.asarray(shape.colors, np.int32)
    colors = (c & 2) | ((c & 1) << 2) | ((c & 4) >> 2)
    return FlatShape(shape.contour_offsets.copy(), pts, shape.types.copy(), colors, shape.inverse_y)


def shifted_frame(shape, w, h, px_range, shift):
    from msdfgen_amd.shape import autoframe
    xf = autoframe(shape.bounds(), int(w), int(h), px_range)
    xf[2] += shift[0]/xf[0]
    xf[3] += shift[1]/xf[1]
    return xf


@functools.lru_cache(maxsize=None)
def variants():
    """{"A": v, "B": v}, v = dict(shapes, xfs (G, 6) for the W x H tile, sizes (G, 2), sized_xfs (G, 6) for the boxes): the 43 glyphs of tests/test_gpu_sized.py
    and their variant B. B's box is the one of the glyph before it (BOXES has 11 entries and 43 = 3 mod 11: every glyph gets another box; the largest width
    and height, hence the slot, stay W x H)."""
    import test_gpu_sized as TS
    shapes, sizes, sized_xfs = TS.glyphs()
    assert (TS.W, TS.H) == (W, H)
    a = {"shapes": list(shapes), "xfs": np.stack([shifted_frame(s, W, H, PX_A, (0, 0)) for s in shapes]), "sizes": sizes.copy(), "sized_xfs": sized_xfs.copy()}
    sb = [mirrored(s) for s in shapes]
    bs = np.roll(sizes, 1, axis=0)
    b = {"shapes": sb, "xfs": np.stack([shifted_frame(s, W, H, PX_B, SHIFT_B) for s in sb]), "sizes": bs,
         "sized_xfs": np.stack([shifted_frame(s, w, h, min(PX_B, .5*min(int(w), int(h))), (0, 0) if min(int(w), int(h)) < 4 else SHIFT_B) for s, (w, h) in zip(sb, bs)])}
    return {"A": a, "B": b}


def repeated(variant, reps):
    """The variant `reps` times over, as tests/test_gpu_sized.py's repeated() does: glyph g is glyph g % 43."""
    v = variants()[variant]
    return {"shapes": list(v["shapes"])*reps, "xfs": np.tile(v["xfs"], (reps, 1)), "sizes": np.tile(v["sizes"], (reps, 1)), "sized_xfs": np.tile(v["sized_xfs"], (reps, 1))}


def rectangles(variant, n_glyphs, channels):
    """(byte offsets (G,), row stride, atlas bytes) of the W x H rectangles of to_bytes: A packs the glyphs in order, B in reverse order and ATLAS_PAD-3 bytes on."""
    tile = W*H*channels
    g = np.arange(n_glyphs, dtype=np.int64)
    off = g*tile if variant == "A" else (n_glyphs-1-g)*tile+ATLAS_PAD-3
    return off, W*channels, n_glyphs*tile+ATLAS_PAD


def bits(a):
    """The bytes of an array (a NaN equals itself, -0 differs from 0)."""
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def equal_glyphs(a, b, n_glyphs):
    """Glyphs whose share of two equally shaped outputs (G leading, or G equal parts of a flat array) has the same bytes in both."""
    x, y = bits(a), bits(b)
    assert x.size == y.size and x.size % n_glyphs == 0, (x.size, y.size, n_glyphs)
    return np.nonzero((x.reshape(n_glyphs, -1) == y.reshape(n_glyphs, -1)).all(axis=1))[0].tolist()


def verdict(what, got, want, stale=None):
    """None if got has want's bytes, else one line: how many bytes differ, where first, and how many of them carry the OTHER variant's value (a read of the
    input that was there before) or the sentinel's."""
    x, y = bits(got), bits(want)
    if x.size != y.size:
        return "%s: %d bytes, expected %d" % (what, x.size, y.size)
    bad = x != y
    if not bad.any():
        return None
    msg = "%s: %d of %d bytes differ, first at byte %d (got 0x%02x, expected 0x%02x)" % (what, int(bad.sum()), x.size, int(np.argmax(bad)), int(x[np.argmax(bad)]),
                                                                                         int(y[np.argmax(bad)]))
    if stale is not None and bits(stale).size == x.size:
        msg += "; %d of them are the other variant's bytes" % int((bad & (x == bits(stale))).sum())
    return msg
