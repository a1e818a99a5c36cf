"""Generates tests/golden/boxes.npz: what the tests of the device's box sizes (Shape::getBounds with border and miters, msdf_frame.hpp: mitersGlyphWave,
boxGlyph, k_box) compare against. Data only, recorded from the compiled reference (oracle/_ref/libmsdfgen_ref.so, made by `make -C oracle`): its own
Shape::getBounds(double, double, int) and Shape::boundMiters, called through ctypes by mangled name (tests/boxcases.py: RefBounds).

    python tools/make_golden_boxes.py

  batch_*      one CSR batch: the shapes of frame.npz's batch set, then the hand-built ones (hand_shapes below: rings of 63, 64 and 1 000 edges, a closed
               one-edge cubic contour, 60 + 8 edges in two contours)
  bounds       [shape][combo][4]: getBounds(border, miterLimit, polarity) over boxcases.MATRIX (3 borders x 5 miter limits x 3 polarities)
  raw_*        the raw outlines of frame.npz; prep_*: what the reference's orientContours, normalize and edgeColoringSimple(3.0, 0) make of them, in the
               reference CLI's order
  raw_plain    getBounds() after normalize (before the colouring)
  raw_bounds   [shape][combo][4]: raw_plain grown by the border, then Shape::boundMiters of the PREPARED shape (boxcases.RefBounds.composed)

The tool refuses to write when a recorded value is NaN, when the miters do not move enough of the batch set's bounds to test anything (border .125, limit 4:
polarity 0 at least 60 of the set's shapes, +1 and -1 at least 30 each, +1 and -1 different on at least one), or unless exactly 4 of the set have no box.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from msdfgen_amd.shape import FlatShape, ShapeBatch  # noqa: E402
from oracle.pyoracle import Ref  # noqa: E402
import boxcases as BC  # noqa: E402
import framecases as FC  # noqa: E402
import geomcases as GC  # noqa: E402
from make_golden_frame import ring  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
W = 7


def star(cx, cy, points, r_out, r_in):
    """2*points linear edges with acute tips: the miters reach far beyond the bounds."""
    v = [(cx+(r_out if k % 2 == 0 else r_in)*np.cos(np.pi*k/points+.3), cy+(r_out if k % 2 == 0 else r_in)*np.sin(np.pi*k/points+.3)) for k in range(2*points)]
    return [(W, v[k], v[(k+1) % len(v)]) for k in range(len(v))]


def hand_shapes():
    """(name, FlatShape): rings (make_golden_frame.ring: linear, quadratic and cubic edges, joins of every kind) that end at lane 62 and lane 63 of the
    first pass; a closed one-edge cubic contour, not normalized (the edge is its own previous edge); 60 + 8 edges in two contours (a contour boundary inside
    a pass; the first contour's cyclic previous edge at lane 59, the second's in the NEXT pass); a ring of 1 000 edges (16 passes)."""
    return [("hand/ring63", ring(63, 3)), ("hand/ring64", ring(64, 4)), ("hand/cubic_loop", FlatShape.from_contours([[(W, (0, 0), (4, 3), (-4, 3), (0, 0))]])),
            ("hand/ring60_star8", FlatShape.from_contours(GC.contours_of(ring(60, 5))+[star(30., 8., 4, 5., 1.25)])), ("hand/ring1000", ring(1000, 6))]


def arrays(prefix, batch):
    return {prefix+"_gco": batch.glyph_contour_offsets, prefix+"_co": batch.contour_offsets, prefix+"_points": batch.points,
            prefix+"_types": batch.types.astype(np.uint8), prefix+"_colors": batch.colors.astype(np.uint8), prefix+"_names": np.array(batch.names)}


def main():
    ref = Ref()
    rb = BC.RefBounds(ref)
    fz, fbatch, fraw = FC.golden()
    n_set = fbatch.n_glyphs
    hand = hand_shapes()
    batch = ShapeBatch.from_shapes(fbatch.shapes()+[s for _, s in hand], list(fbatch.names)+[n for n, _ in hand])
    bounds = np.stack([rb.matrix(batch.shape(g)) for g in range(batch.n_glyphs)])
    plain = bounds[:, BC.combo(0., 0., 0)]
    if (plain[:n_set].view(np.uint64) != fz["batch_bounds"].view(np.uint64)).any():
        sys.exit("make_golden_boxes: getBounds(0, 0, 0) by mangled name differs from frame.npz's bounds: the binding is wrong")

    prepared, raw_plain, raw_bounds = [], [], []
    for g in range(fraw.n_glyphs):
        h, p = BC.ref_raw(ref, fraw.shape(g))
        fa = ref.flatten(h)
        prepared.append(FlatShape(fa.contour_offsets, fa.points, fa.types, fa.colors))
        raw_plain.append(p)
        raw_bounds.append(np.stack([rb.composed(p, h, b, m, pol) for (b, m, pol) in BC.MATRIX]))
        ref.free(h)
    raw_plain, raw_bounds = np.stack(raw_plain), np.stack(raw_bounds)
    prep = ShapeBatch.from_shapes(prepared, list(fraw.names))

    if np.isnan(bounds).any() or np.isnan(raw_bounds).any() or np.isnan(raw_plain).any():
        sys.exit("make_golden_boxes: a recorded value is NaN")
    border_only = bounds[:n_set, BC.combo(.125, 0., 0)]
    moved = {p: (bounds[:n_set, BC.combo(.125, 4., p)].view(np.uint64) != border_only.view(np.uint64)).any(1) for p in BC.POLARITIES}
    counts = [int(moved[p].sum()) for p in (0, 1, -1)]
    differ = int((bounds[:n_set, BC.combo(.125, 4., 1)].view(np.uint64) != bounds[:n_set, BC.combo(.125, 4., -1)].view(np.uint64)).any(1).sum())
    limit1 = int((bounds[:n_set, BC.combo(.125, 1., 0)].view(np.uint64) != border_only.view(np.uint64)).any(1).sum())
    boxless = int(BC.no_box(plain[:n_set]).sum())
    print("of %d shapes at border .125, limit 4: polarity 0 moves %d, +1 moves %d, -1 moves %d; +1 and -1 differ on %d; limit 1 moves %d; %d have no box"
          % (n_set, counts[0], counts[1], counts[2], differ, limit1, boxless))
    if counts[0] < 60 or counts[1] < 30 or counts[2] < 30 or differ < 1:
        sys.exit("make_golden_boxes: the miters move too few bounds to test anything")
    if boxless != 4:
        sys.exit("make_golden_boxes: %d shapes of the set have no box, expected 4" % boxless)

    path = os.path.join(GOLDEN, "boxes.npz")
    np.savez_compressed(path, n_set=np.int32(n_set), matrix=np.array(BC.MATRIX, np.float64), bounds=bounds, raw_plain=raw_plain, raw_bounds=raw_bounds,
                        **arrays("batch", batch), **arrays("raw", fraw), **arrays("prep", prep))
    print("boxes.npz: %d array shapes (%d edges), %d raw outlines, %d combos, %d bytes" % (batch.n_glyphs, batch.n_edges, fraw.n_glyphs, len(BC.MATRIX), os.path.getsize(path)))


if __name__ == "__main__":
    main()
