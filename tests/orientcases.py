"""Shapes and the reference sequence for the orientation tests (test_cabi_prepare_orient.py, test_gpu_prepare_orient.py): the hand-built cases of
Shape::orientContours' branches, the perturbations of a glyph set (contours reversed), and what the reference CLI runs on a glyph --
orientContours, normalize, the winding step, the colouring (main.cpp:1105-1143, 1255) -- through the compiled reference (oracle/_ref)."""
import math

import numpy as np

from msdfgen_amd.shape import FlatShape, ShapeBatch

WHITE = 7
RATIO = .5*(math.sqrt(5)-1)          # Shape.cpp:156


def reverse_edges(points, types, colors, b, e):
    """Contour::reverse (core/Contour.cpp:83-88) of the edges [b, e) of flat arrays, in place: edge order and every edge's control points; colours
    travel with their edges."""
    if e <= b:
        return
    p, t, c = points[b:e][::-1].copy(), types[b:e][::-1].copy(), colors[b:e][::-1].copy()
    out = np.zeros_like(p)
    for k in range(len(t)):
        cp = p[k].reshape(4, 2)[:int(t[k])+1][::-1]
        out[k, :cp.size] = cp.reshape(-1)
    points[b:e], types[b:e], colors[b:e] = out, t, c


def perturbed(batch: ShapeBatch, seed=5) -> ShapeBatch:
    """Every contour of every 3rd glyph reversed; one seeded contour reversed in every 5th glyph."""
    pts, types, colors = batch.points.copy(), batch.types.copy(), batch.colors.copy()
    gco, co = batch.glyph_contour_offsets, batch.contour_offsets
    rng = np.random.default_rng(seed)
    for g in range(batch.n_glyphs):
        c0, c1 = int(gco[g]), int(gco[g+1])
        if g % 3 == 0:
            for c in range(c0, c1):
                reverse_edges(pts, types, colors, int(co[c]), int(co[c+1]))
        if g % 5 == 0 and c1 > c0:
            c = int(rng.integers(c0, c1))
            reverse_edges(pts, types, colors, int(co[c]), int(co[c+1]))
    return ShapeBatch(gco.copy(), co.copy(), pts, types, colors, np.asarray(batch.inverse_y).copy(), list(batch.names or []))


def wiped(batch: ShapeBatch) -> ShapeBatch:
    return ShapeBatch(batch.glyph_contour_offsets, batch.contour_offsets, batch.points, batch.types, np.full(batch.n_edges, WHITE, np.int32),
                      batch.inverse_y, batch.names)


def _L(a, b):
    return (WHITE, a, b)


def _poly(pts):
    return [_L(pts[i], pts[(i+1) % len(pts)]) for i in range(len(pts))]


def _rect(x0, y0, x1, y1, ccw=True):
    pts = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]          # starts with a horizontal edge: the y1 search goes past it
    return _poly(pts if ccw else pts[:1]+pts[1:][::-1])


def hand_built():
    """(name, FlatShape): the branches of orientContours and the sizes past its LDS tier."""
    r = RATIO
    cases = []
    cases.append(("first-edges-horizontal", FlatShape.from_contours([_poly([(0, 0), (1, 0), (2, 0), (2, 2), (0, 2)]),
                                                                      _poly([(.5, .5), (.5, 1.5), (1.5, 1.5), (1.5, .5)])])))
    # every end point on y = 0: the scanline comes from point(ratio) (Shape.cpp:165-166)
    cases.append(("all-horizontal", FlatShape.from_contours([[(WHITE, (0, 0), (1, 2), (2, 0)), (WHITE, (2, 0), (1, -1), (0, 0))],
                                                             [(WHITE, (3, 0), (4, -1), (5, 0)), (WHITE, (5, 0), (4, 2), (3, 0))]])))
    # the first contour's scanline is y = ratio exactly; two triangles share the vertex (3, ratio): a tie at x = 3, both directions zeroed
    cases.append(("shared-vertex-tie", FlatShape.from_contours([_rect(0, 0, 1, 1),
                                                                _poly([(2, 0), (3, r), (2, 1)]), _poly([(4, 0), (4, 1), (3, r)]),
                                                                _poly([(6, 0), (7, r), (6, 1)]), _poly([(7, r), (8, 1), (8, 0)])])))
    cases.append(("nested-3-deep", FlatShape.from_contours([_rect(0, 0, 10, 10), _rect(1, 1, 9, 9, True), _rect(2, 2, 8, 8, False),
                                                            _rect(3, 3, 7, 7, False), _rect(4, 4, 6, 6)])))
    circle = lambda cx, cy, rad, ccw: [(WHITE, (cx+rad*math.cos(a), cy+rad*math.sin(a)), (cx+rad/math.cos(math.pi/8)*math.cos(a+s*math.pi/8),
                                                                                       cy+rad/math.cos(math.pi/8)*math.sin(a+s*math.pi/8)),
                                        (cx+rad*math.cos(a+s*math.pi/4), cy+rad*math.sin(a+s*math.pi/4)))
                                       for s in [1 if ccw else -1] for a in [s*k*math.pi/4 for k in range(8)]]
    cases.append(("overlapping", FlatShape.from_contours([circle(0, 0, 2, True), circle(1.5, .3, 2, False), circle(.7, 1.1, 1.2, True)])))
    cases.append(("empty-contours", FlatShape.from_contours([[], _rect(0, 0, 2, 1, False), [], _rect(.5, .2, 1, .8), []])))
    cases.append(("only-empty-contours", FlatShape.from_contours([[], []])))
    cases.append(("no-contours", FlatShape.from_contours([])))
    # single-edge contours (a cubic loop; a quadratic running out and back): orientation sees them before splitInThirds
    cases.append(("single-edge", FlatShape.from_contours([[(WHITE, (0, 0), (4, 3), (-4, 3), (0, 0))], [(WHITE, (5, 0), (2, 3), (8, 3), (5, 0))],
                                                          _rect(-1, -1, 9, 4, False)])))
    n = 2100
    big = _poly([(10*math.cos(2*math.pi*k/n), 10*math.sin(-2*math.pi*k/n)) for k in range(n)])
    cases.append(("2100-edge-contour", FlatShape.from_contours([big, _rect(-3, -3, 3, 3, False)])))
    # 600 thin rectangles in one row: the first scanline has 1 200 hits (past the LDS tier) and votes on 600 contours (past the LDS votes)
    row = [_rect(3*k, 0, 3*k+1, 1, ccw=(k % 3 != 0)) for k in range(600)]
    cases.append(("hits-past-lds", FlatShape.from_contours(row)))
    # 30 x 30 squares: 900 contours, a scanline per row
    grid = [_rect(2*i, 2*j, 2*i+1, 2*j+1, ccw=((i*7+j*3) % 4 != 0)) for j in range(30) for i in range(30)]
    cases.append(("900-contours", FlatShape.from_contours(grid)))
    return cases


def hand_built_batch() -> ShapeBatch:
    cases = hand_built()
    return ShapeBatch.from_shapes([s for _, s in cases], [n for n, _ in cases])


def ref_prepare(ref, shape, orient=False, winding=0, normalize=True, coloring=1, angle=3.0, seed=0):
    """The reference's own sequence on a copy of `shape` -> FlatArrays: orientContours, normalize, the winding step (reversal restated in numpy: it only
    moves values), the colouring."""
    h = ref.shape_from_flat(shape)
    if orient:
        ref.lib.ref_shape_orient_contours(h)
    if normalize:
        ref.lib.ref_shape_normalize(h)
    if winding:
        rev = winding == 1
        if winding == 2:
            b = ref.bounds(h)
            rev = ref.shape_distance(h, 1, False, [(b[0]-(b[2]-b[0])-1, b[1]-(b[3]-b[1])-1)])[0, 0] > 0
        if rev:
            fa = ref.flatten(h)
            ref.free(h)
            pts, types, colors = fa.points.copy(), fa.types.copy(), fa.colors.copy()
            for c in range(len(fa.contour_offsets)-1):
                reverse_edges(pts, types, colors, int(fa.contour_offsets[c]), int(fa.contour_offsets[c+1]))
            h = ref.shape_from_flat(FlatShape(fa.contour_offsets, pts, types, colors, fa.inverse_y))
    if coloring == 1:
        ref.lib.ref_shape_color_simple(h, angle, seed)
    elif coloring == 2:
        ref.lib.ref_shape_color_inktrap(h, angle, seed)
    fa = ref.flatten(h)
    ref.free(h)
    return FlatShape(fa.contour_offsets, fa.points, fa.types, fa.colors, fa.inverse_y)


def ref_prepare_batch(ref, batch: ShapeBatch, orient=False, winding=0, normalize=True, coloring=1, angle=3.0, seeds=None) -> ShapeBatch:
    return ShapeBatch.from_shapes([ref_prepare(ref, batch.shape(g), orient, winding, normalize, coloring, angle, 0 if seeds is None else int(seeds[g]))
                                   for g in range(batch.n_glyphs)], list(batch.names or []))


def same_batch(a: ShapeBatch, b: ShapeBatch, what):
    """Offsets, types, colours and control points bit for bit."""
    assert (np.asarray(a.glyph_contour_offsets) == np.asarray(b.glyph_contour_offsets)).all(), what+": glyph offsets"
    assert len(a.contour_offsets) == len(b.contour_offsets) and (np.asarray(a.contour_offsets) == np.asarray(b.contour_offsets)).all(), what+": contour offsets"
    assert (np.asarray(a.types) == np.asarray(b.types)).all(), what+": types"
    assert (np.asarray(a.colors) == np.asarray(b.colors)).all(), what+": colours"
    pa, pb = np.ascontiguousarray(a.points, np.float64).view(np.uint64), np.ascontiguousarray(b.points, np.float64).view(np.uint64)
    assert pa.shape == pb.shape and (pa == pb).all(), what+": %d control-point values differ bitwise" % int((pa != pb).sum())
