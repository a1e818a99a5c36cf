"""Generates tests/golden/legacy.npz: what the tests of the legacy generators and the legacy error correction (msdf_legacy.hpp) compare against.
Needs the compiled reference (oracle/_ref/libmsdfgen_ref.so and the reference's own CLI oracle/_ref/cli/msdfgen_cpu, both made by `make -C oracle`).

    python tools/make_golden_legacy.py

Where the values come from
  generators   the reference's own generateSDF_legacy / generatePSDF_legacy / generateMSDF_legacy / generateMTSDF_legacy, called through ctypes by
               mangled name (tests/legacycases.py: RefLegacy). Before anything is recorded the binding has to reproduce, byte for byte, files the
               reference CLI writes (`<mode> -legacy -noscanline -format fl32` on pre-coloured shape descriptions, which the CLI does not colour
               again): every mode, every correction mode, a Y-downward shape, an asymmetric scale and range. The tool aborts otherwise.
  default flow the CLI's `-legacy` without -noscanline (legacy field -> distanceSignCorrection -> msdfErrorCorrection without the distance check,
               main.cpp:1223-1298): its fl32 files as they are.
  stencils     ErrorCorrectionConfig::buffer handed to generateMSDF_legacy, for the four combinations of the shape's and the bitmap's orientation.
  correction   msdfErrorCorrection_legacy on seeded random fields. A plain restatement of its two passes in numpy must agree with the reference, and
               shows for every field of at least 2x2 that some texel ends up different from what the second pass alone makes of the input: the
               second pass really reads what the first one wrote. The seed is searched until that holds.

What is recorded: the shapes (one CSR batch), per record the six transform doubles (sx, sy, tx, ty, range lower, range upper), the inputs and the
expected outputs in memory-row order. Nothing of the reference's text.

Shapes: shape_a (linear), DejaVu '@' of latin.npz (quadratic), the outline tests/test_gpu_cli.py calls TEARDROP and the cubic teardrop of the
reference's README, the five-contour BLOBS, the lattice_ties and coincident families of tests/geomcases.py (the first edge in shape order must win a
tie), the empty shape, a contour coloured YELLOW only (no edge serves blue: the channel stays at -DBL_MAX), the 65- and 129-edge rings of frame.npz
(coloured here), and shape_a Y-downward. The empty and the YELLOW shape are recorded with the correction DISABLED (the raw field with its non-finite
channels) and under the correction modes the public defaults would run over them (a correction pass over infinities).
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from msdfgen_amd.shape import FlatShape, ShapeBatch, autoframe  # noqa: E402
from oracle.pyoracle import Ref  # noqa: E402
import framecases as FC  # noqa: E402
import geomcases as GC  # noqa: E402
import legacycases as LC  # noqa: E402
from test_gpu_cli import BLOBS, TEARDROP  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "oracle", "_ref", "cli", "msdfgen_cpu")
MODE_NAMES = {1: "sdf", 2: "psdf", 3: "msdf", 4: "mtsdf"}
EC_NAMES = {0: "disabled", 1: "distance-fast", 2: "auto-fast", 3: "edge-fast"}          # ErrorCorrectionConfig::Mode -> -errorcorrection (main.cpp:864-895)
COLOUR_LETTERS = {3: "y", 5: "m", 6: "c", 7: "w"}
Y, W = 3, 7


def describe(shape):
    """msdfgen's shape description of a FlatShape WITH its colours (so that the CLI keeps them) and its Y orientation; repr round-trips."""
    pt = lambda p, i: "%r, %r" % (float(p[2*i]), float(p[2*i+1]))
    out = ["@y-down" if shape.inverse_y else "@y-up"]
    for c in range(shape.n_contours):
        e0, e1 = int(shape.contour_offsets[c]), int(shape.contour_offsets[c+1])
        parts = []
        for e in range(e0, e1):
            p, t = shape.points[e], int(shape.types[e])
            parts.append(pt(p, 0))
            parts.append(COLOUR_LETTERS[int(shape.colors[e])]+("("+"; ".join(pt(p, i) for i in range(1, t))+")" if t > 1 else ""))
        if e1 > e0:
            parts.append(pt(shape.points[e1-1], int(shape.types[e1-1])))
        out.append("{ "+"; ".join(parts)+" }")
    return "\n".join(out)+"\n"


def flat_of(ref, h, inverse_y=False):
    fa = ref.flatten(h)
    return FlatShape(fa.contour_offsets, fa.points, fa.types, fa.colors, inverse_y)


def prepared(ref, text=None, shape=None, normalize=True):
    """What the CLI makes of an uncoloured outline: Shape::normalize, edgeColoringSimple(3.0, 0) (main.cpp:1125, 1255)."""
    h = ref.shape_from_desc(text) if text is not None else ref.shape_from_flat(shape)
    ref.prepare(h, angle=3.0, seed=0, normalize=normalize, color=True)
    s = flat_of(ref, h)
    ref.free(h)
    return s


def assert_normalized(ref, shape, name):
    """The CLI normalizes what it reads: the recorded shapes must come through Shape::normalize unchanged."""
    h = ref.shape_from_flat(shape)
    ref.lib.ref_shape_normalize(h)
    again = flat_of(ref, h)
    ref.free(h)
    same = (np.array_equal(again.contour_offsets, shape.contour_offsets) and np.array_equal(again.types, shape.types) and
            np.array_equal(again.points.view(np.uint64), shape.points.view(np.uint64)))
    if not same:
        sys.exit("make_golden_legacy: Shape::normalize changes %s; the CLI would render another shape" % name)


def cli(tmp, shape, mode, w, h, xf, ec=None, noscanline=True):
    """The CLI's fl32 output (memory rows upward = file order) for a pre-coloured description."""
    desc, out = os.path.join(tmp, "shape.txt"), os.path.join(tmp, "out.fl32")
    with open(desc, "w") as f:
        f.write(describe(shape))
    cmd = [CLI, MODE_NAMES[mode], "-legacy", "-format", "fl32", "-shapedesc", desc, "-dimensions", str(w), str(h), "-ascale", repr(float(xf[0])), repr(float(xf[1])),
           "-translate", repr(float(xf[2])), repr(float(xf[3])), "-arange", repr(float(xf[4])), repr(float(xf[5])), "-o", out]
    if noscanline:
        cmd.append("-noscanline")
    if ec is not None:
        cmd += ["-errorcorrection", EC_NAMES[ec]]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("make_golden_legacy: %s failed: %s %s" % (" ".join(cmd), r.stdout, r.stderr))
    raw = open(out, "rb").read()
    n = LC.CHANNELS[mode]
    assert raw[:4] == b"FL32" and len(raw) == 16+4*w*h*n, (len(raw), w, h, n)
    return np.frombuffer(raw[16:], np.float32).reshape(h, w, n).copy()


def frames(ref, shape, w, h):
    """(autoframe, one with sx != sy, one with an asymmetric range) for a w x h bitmap; a pixel range that still fits the smallest bitmaps."""
    hd = ref.shape_from_flat(shape)
    b = ref.bounds(hd)
    ref.free(hd)
    px = 4. if min(w, h) > 4 else .5
    auto = autoframe(b, w, h, px)
    skew = auto.copy()
    skew[1] *= .8125
    asym = auto.copy()
    asym[4], asym[5] = -.7*auto[5], 1.2*auto[5]
    return auto, skew, asym


# ---- msdfErrorCorrection_legacy restated (only to show that its second pass depends on its first) ----------------------------------------

def clash(a, b, threshold):
    f, ab = np.float32, lambda x: np.float32(abs(x))
    a0, a1, a2, b0, b1, b2 = f(a[0]), f(a[1]), f(a[2]), f(b[0]), f(b[1]), f(b[2])
    if ab(b0-a0) < ab(b1-a1):
        a0, a1, b0, b1 = a1, a0, b1, b0
    if ab(b1-a1) < ab(b2-a2):
        a1, a2, b1, b2 = a2, a1, b2, b1
        if ab(b0-a0) < ab(b1-a1):
            a0, a1, b0, b1 = a1, a0, b1, b0
    return bool(float(ab(b1-a1)) >= threshold and not (b0 == b1 and b0 == b2) and ab(a2-f(.5)) >= ab(b2-f(.5)))


def clash_pass(field, diagonal, tx, ty):
    h, w, _ = field.shape
    out = field.copy()
    steps = [(-1, -1, tx+ty), (1, -1, tx+ty), (-1, 1, tx+ty), (1, 1, tx+ty)] if diagonal else [(-1, 0, tx), (1, 0, tx), (0, -1, ty), (0, 1, ty)]
    for y in range(h):
        for x in range(w):
            if any(0 <= x+dx < w and 0 <= y+dy < h and clash(field[y, x], field[y+dy, x+dx], t) for dx, dy, t in steps):
                out[y, x, :3] = sorted(field[y, x, :3])[1]
    return out


def correction_fields(rl):
    fields = []
    for n in (3, 4):
        for (w, h) in LC.EC_SIZES:
            for (tx, ty) in LC.EC_THRESHOLDS:
                for seed in range(1000):
                    field = np.random.default_rng([n, w, h, int(tx*10), seed]).uniform(0, 1, (h, w, n)).astype(np.float32)
                    want = rl.correction(field, tx, ty)
                    both = clash_pass(clash_pass(field, False, tx, ty), True, tx, ty)
                    if (both.view(np.uint32) != want.view(np.uint32)).any():
                        sys.exit("make_golden_legacy: the numpy restatement of msdfErrorCorrection_legacy disagrees with the reference")
                    second_only = clash_pass(field, True, tx, ty)
                    if min(w, h) < 2 or (second_only.view(np.uint32) != want.view(np.uint32)).any():
                        break
                else:
                    sys.exit("make_golden_legacy: no seed makes pass 2 depend on pass 1 at %dx%d" % (w, h))
                if n == 4:
                    assert (want[..., 3].view(np.uint32) == field[..., 3].view(np.uint32)).all()
                fields.append(LC.EcRecord(n, w, h, tx, ty, field, want))
    return fields


def main():
    ref = Ref()
    rl = LC.RefLegacy(ref)
    za = np.load(os.path.join(GOLDEN, "shape_a.npz"))
    shape_a = FlatShape(za["contour_offsets"], za["points"], za["types"], za["colors"])
    zl = np.load(os.path.join(GOLDEN, "latin.npz"))
    latin = ShapeBatch(zl["glyph_contour_offsets"].astype(np.int32), zl["contour_offsets"].astype(np.int32), zl["points"], zl["types"].astype(np.int32),
                       zl["colors"].astype(np.int32), zl["inverse_y"], [str(n) for n in zl["names"]])
    at = latin.shape(latin.names.index("U+0040"))
    _, fbatch, _ = FC.golden()
    fnames = list(fbatch.names)
    cubic_teardrop = prepared(ref, shape=fbatch.shape(fnames.index("norm/teardrop")), normalize=False)
    rings = [prepared(ref, shape=fbatch.shape(fnames.index("hand/ring%d" % n)), normalize=False) for n in (65, 129)]
    assert [r.n_edges for r in rings] == [65, 129]
    yellow = FlatShape.from_contours([[(Y, (1, 1), (9, 2)), (Y, (9, 2), (8, 5), (5, 8)), (Y, (5, 8), (1, 1))]])
    shapes = [("shape_a", shape_a), ("latin/U+0040", at), ("cli_teardrop", prepared(ref, text=TEARDROP)), ("cubic_teardrop", cubic_teardrop),
              ("blobs", prepared(ref, text=BLOBS)), ("empty", FlatShape.from_contours([])), ("yellow", yellow), ("ring65", rings[0]), ("ring129", rings[1]),
              ("shape_a_ydown", FlatShape(shape_a.contour_offsets, shape_a.points, shape_a.types, shape_a.colors, True))]
    geom = [c for c in GC.cases(("lattice_ties", "coincident")) if c.w <= 40 and c.h <= 32]
    shapes += [("geom/"+c.name, c.shape) for c in geom]
    names = [n for n, _ in shapes]
    index = {n: k for k, n in enumerate(names)}
    by_name = dict(shapes)
    for n in ("shape_a", "latin/U+0040", "cli_teardrop", "cubic_teardrop", "blobs", "shape_a_ydown"):
        assert_normalized(ref, by_name[n], n)

    with tempfile.TemporaryDirectory() as tmp:
        # 1. the binding reproduces the CLI
        proofs = [("shape_a", 3, 40, 32, 0, 2), ("blobs", 4, 9, 17, 1, 1), ("cubic_teardrop", 2, 7, 5, 0, None), ("latin/U+0040", 1, 8, 8, 2, None),
                  ("shape_a_ydown", 3, 9, 17, 2, 3), ("cli_teardrop", 4, 40, 32, 0, 0), ("blobs", 3, 40, 32, 2, 2)]
        for name, mode, w, h, frame, ec in proofs:
            s = by_name[name]
            xf = frames(ref, s, w, h)[frame]
            want = cli(tmp, s, mode, w, h, xf, ec)
            got = rl.generate(s, mode, w, h, xf, ec_mode=ec if ec is not None else 2)
            if want.tobytes() != got.tobytes():
                sys.exit("make_golden_legacy: the ctypes binding does not reproduce the CLI for %s (%s, %dx%d): %d floats differ"
                         % (name, MODE_NAMES[mode], w, h, int((want.view(np.uint32) != got.view(np.uint32)).sum())))
        print("binding proven on %d CLI files" % len(proofs))

        records = []

        def add(label, name, mode, w, h, xf, ec=2, y_down=False, stencil=False):
            s = by_name[name]
            st = np.zeros((h, w), np.uint8) if stencil else None
            out = rl.generate(s, mode, w, h, xf, ec_mode=ec, y_down=y_down, stencil=st)
            records.append(LC.Record(label, index[name], mode, w, h, np.asarray(xf, np.float64), ec if mode >= 3 else 0, y_down, False, 0, .5, out, st))

        big = LC.SIZES[-1]
        for mode in (1, 2, 3, 4):                                            # every mode; every size
            add("shape_a/%s" % MODE_NAMES[mode], "shape_a", mode, big[0], big[1], frames(ref, shape_a, *big)[0])
        for (w, h) in LC.SIZES[:-1]:
            add("shape_a/msdf/%dx%d" % (w, h), "shape_a", 3, w, h, frames(ref, shape_a, w, h)[0])
            add("blobs/mtsdf/%dx%d" % (w, h), "blobs", 4, w, h, frames(ref, by_name["blobs"], w, h)[0], ec=1)
        add("at/msdf/skewed", "latin/U+0040", 3, 9, 17, frames(ref, at, 9, 17)[1])                     # every transform
        add("at/mtsdf/asymmetric", "latin/U+0040", 4, big[0], big[1], frames(ref, at, *big)[2])
        add("at/psdf/skewed", "latin/U+0040", 2, 7, 5, frames(ref, at, 7, 5)[1])
        add("at/sdf/asymmetric", "latin/U+0040", 1, 8, 8, frames(ref, at, 8, 8)[2])
        for ec in (0, 1, 2, 3):                                              # every correction mode, on cubics
            add("cubic_teardrop/msdf/ec%d" % ec, "cubic_teardrop", 3, big[0], big[1], frames(ref, cubic_teardrop, *big)[0], ec=ec)
            add("blobs/mtsdf/ec%d" % ec, "blobs", 4, 9, 17, frames(ref, by_name["blobs"], 9, 17)[2], ec=ec)
        add("cubic_teardrop/psdf", "cubic_teardrop", 2, 9, 17, frames(ref, cubic_teardrop, 9, 17)[0])
        add("cli_teardrop/msdf", "cli_teardrop", 3, big[0], big[1], frames(ref, by_name["cli_teardrop"], *big)[1])
        add("blobs/msdf", "blobs", 3, big[0], big[1], frames(ref, by_name["blobs"], *big)[0])
        for k, c in enumerate(geom):                                         # ties: the first edge in shape order wins, in every mode
            add(c.name, "geom/"+c.name, (3, 4, 2, 1)[k % 4], c.w, c.h, c.xf, y_down=c.y_down)
        for mode in (1, 2, 3, 4):
            add("empty/%s" % MODE_NAMES[mode], "empty", mode, 7, 5, frames(ref, by_name["empty"], 7, 5)[0], ec=0)
        add("yellow/msdf", "yellow", 3, 9, 17, frames(ref, yellow, 9, 17)[0], ec=0)
        add("yellow/mtsdf", "yellow", 4, 8, 8, frames(ref, yellow, 8, 8)[0], ec=0)
        assert not np.isfinite(records[-1].out[..., 2]).any() and np.isfinite(records[-1].out[..., (0, 1, 3)]).all()
        add("yellow/msdf/ec2", "yellow", 3, 9, 17, frames(ref, yellow, 9, 17)[0], ec=2)            # the correction over a channel of infinities
        add("yellow/mtsdf/ec1", "yellow", 4, 8, 8, frames(ref, yellow, 8, 8)[0], ec=1, y_down=True)
        add("empty/msdf/ec2", "empty", 3, 7, 5, frames(ref, by_name["empty"], 7, 5)[0], ec=2)
        add("empty/mtsdf/ec3", "empty", 4, 7, 5, frames(ref, by_name["empty"], 7, 5)[0], ec=3)
        add("ring65/msdf", "ring65", 3, big[0], big[1], frames(ref, rings[0], *big)[0])
        add("ring129/mtsdf", "ring129", 4, big[0], big[1], frames(ref, rings[1], *big)[0])
        add("shape_a_ydown/msdf", "shape_a_ydown", 3, 9, 17, frames(ref, shape_a, 9, 17)[0])
        add("shape_a_ydown/sdf/ydown", "shape_a_ydown", 1, 7, 5, frames(ref, shape_a, 7, 5)[0], y_down=True)
        # 2. stencils: inverse_y x y_orientation at 9 x 7
        for name in ("shape_a", "shape_a_ydown"):
            for y_down in (False, True):
                add("stencil/%s/%s" % (name, "ydown" if y_down else "yup"), name, 3, 9, 7, frames(ref, shape_a, 9, 7)[0], y_down=y_down, stencil=True)
                assert records[-1].stencil.any()
        # 3. the CLI's default -legacy flow (scanline pass on)
        blobs = by_name["blobs"]
        xf = frames(ref, blobs, *big)[0]
        zero = float(np.float32(xf[4]/(xf[4]-xf[5])))                          # main.cpp:1282
        for mode in (3, 4):
            out = cli(tmp, blobs, mode, big[0], big[1], xf, None, noscanline=False)
            raw = rl.generate(blobs, mode, big[0], big[1], xf, ec_mode=0)
            assert (out.view(np.uint32) != raw.view(np.uint32)).any(), "the default flow changes nothing: not a test of it"
            records.append(LC.Record("default_flow/%s" % MODE_NAMES[mode], index["blobs"], mode, big[0], big[1], xf, 2, False, True, 0, zero, out, None))

    fields = correction_fields(rl)
    batch = ShapeBatch.from_shapes([s for _, s in shapes], names)
    rec_off = np.cumsum([0]+[r.out.size for r in records])[:-1]
    st_sizes = [r.stencil.size if r.stencil is not None else 0 for r in records]
    st_off = np.where(np.array(st_sizes) > 0, np.cumsum([0]+st_sizes)[:-1], -1)
    ec_off = np.cumsum([0]+[f.field.size for f in fields])[:-1]
    np.savez_compressed(
        os.path.join(GOLDEN, "legacy.npz"), shapes_gco=batch.glyph_contour_offsets, shapes_co=batch.contour_offsets, shapes_points=batch.points,
        shapes_types=batch.types.astype(np.uint8), shapes_colors=batch.colors.astype(np.uint8), shapes_inverse_y=batch.inverse_y, shapes_names=np.array(names),
        rec_name=np.array([r.name for r in records]), rec_shape=np.array([r.shape for r in records], np.int32), rec_mode=np.array([r.mode for r in records], np.int32),
        rec_w=np.array([r.w for r in records], np.int32), rec_h=np.array([r.h for r in records], np.int32), rec_xf=np.stack([r.xf for r in records]),
        rec_ec=np.array([r.ec for r in records], np.int32), rec_ydown=np.array([r.y_down for r in records], np.uint8),
        rec_sign=np.array([r.sign for r in records], np.uint8), rec_fill=np.array([r.fill for r in records], np.int32),
        rec_zero=np.array([r.zero for r in records], np.float32), rec_off=rec_off.astype(np.int64), rec_out=np.concatenate([r.out.reshape(-1) for r in records]),
        rec_stencil_off=st_off.astype(np.int64), rec_stencils=np.concatenate([r.stencil.reshape(-1) for r in records if r.stencil is not None]),
        ec_n=np.array([f.n for f in fields], np.int32), ec_w=np.array([f.w for f in fields], np.int32), ec_h=np.array([f.h for f in fields], np.int32),
        ec_tx=np.array([f.tx for f in fields]), ec_ty=np.array([f.ty for f in fields]), ec_off=ec_off.astype(np.int64),
        ec_in=np.concatenate([f.field.reshape(-1) for f in fields]), ec_out=np.concatenate([f.out.reshape(-1) for f in fields]))
    print("legacy.npz: %d shapes (%d edges), %d generator records (%d floats), %d correction fields, %d bytes"
          % (batch.n_glyphs, batch.n_edges, len(records), sum(r.out.size for r in records), len(fields), os.path.getsize(os.path.join(GOLDEN, "legacy.npz"))))


if __name__ == "__main__":
    main()
