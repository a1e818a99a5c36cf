"""Outlines other than synth's for the parity tests (test_geom_cases.py on the CPU, test_gpu_geometry.py on the GPU, fuzzlib's geometry=): the sibling of
xformcases.py, which varies how a glyph is framed. Here the OUTLINE is what a random-coordinate blob never is: texel centres equidistant from edges that
are not neighbours, texel centres on the outline, contours that coincide, edges that degenerate, channels no edge serves, scanlines through vertices
and along horizontal edges, features thinner than a texel.

A case is (name, shape, w, h, xf, y_down) as in xformcases. Coordinates are integers or small dyadic fractions and the framing is a power-of-two scale
s with translation -1/(2s), so that texel centre (x+.5, y+.5) is the shape point ((x+1)/s, (y+1)/s) exactly: every premise is an exact statement in
fp64. Where a premise is about distances (lattice_ties, on_outline) check_premise() evaluates it from the oracle's per-edge signed distances instead of
assuming it; where it is about the outline itself (shared vertices of coincident, the degenerate forms, the colour census of sparse_colours, the rows of
scanline_hits, the contour boxes of slivers) it is computed from the coordinates and colours, which is what those families mean. MIN_COUNT states, per
case, how many texels, rows or vertices are found at the case's own size (families without an entry: at least one); a re-framing at a larger bitmap (cases(w=, h=)) keeps those lattice points."""
import ctypes as C
from collections import namedtuple

import numpy as np

from msdfgen_amd.shape import FlatShape, autoframe

Case = namedtuple("Case", "name shape w h xf y_down")

FAMILIES = ("lattice_ties", "on_outline", "coincident", "degenerate_edges", "sparse_colours", "scanline_hits", "slivers")
BIG_SIZES = ((41, 27), (64, 64))
K, R, G, Y, B, M, CY, W = range(8)                            # EdgeColor: BLACK RED GREEN YELLOW BLUE MAGENTA CYAN WHITE
# A quadratic that runs out and straight back over itself: the sign of its distance is last-ulp noise of acos / cos. The CPU tests keep
# it (the host build uses libm like the oracle); the GPU tests treat it as test_backtracking_curves_... does and keep it out of the bit-exact set.
SIGN_NOISE = ("degenerate_edges/quad_fold_back",)


def rect(x0, y0, x1, y1, cols=(CY, M, Y, CY), flip=False):
    p = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    if flip:
        p = p[::-1]
    return [(cols[k], p[k], p[(k+1) % 4]) for k in range(4)]


def poly(pts, cols=(CY, M, Y)):
    return [(cols[k % len(cols)], pts[k], pts[(k+1) % len(pts)]) for k in range(len(pts))]


def lattice_xf(scale=1., pr=4.):
    """Texel centre (x+.5, y+.5) -> shape point ((x+1)/scale, (y+1)/scale); a range of pr texels."""
    return np.array([scale, scale, -.5/scale, -.5/scale, -.5*pr/scale, .5*pr/scale])


def grid(nx, ny, size, pitch, x0=2, cols=((CY, M, Y, CY), (Y, CY, M, Y), (M, Y, CY, M))):
    return [rect(x0+i*pitch, x0+j*pitch, x0+i*pitch+size, x0+j*pitch+size, cols=cols[(i+2*j) % len(cols)]) for j in range(ny) for i in range(nx)]


DIAMOND = poly([(8, 2), (14, 8), (8, 14), (2, 8)], (CY, M, Y, M))
QUAD_SIDES = [(CY, (2, 4), (7, 0), (12, 4)), (M, (12, 4), (12, 10)), (Y, (12, 10), (7, 14), (2, 10)), (M, (2, 10), (2, 4))]
CUBIC_SIDES = [(CY, (2, 4), (4, 1), (10, 1), (12, 4)), (M, (12, 4), (12, 10)), (Y, (12, 10), (10, 13), (4, 13), (2, 10)), (M, (2, 10), (2, 4))]
QUAD_LENS_L = [(CY, (2, 2), (6, 5), (2, 8)), (M, (2, 8), (2, 2))]             # mirror images about x = 7, the right one walked the other way round
QUAD_LENS_R = [(Y, (12, 8), (8, 5), (12, 2)), (CY, (12, 2), (12, 8))]
CUBIC_LENS_L = [(CY, (2, 2), (6, 3), (6, 7), (2, 8)), (M, (2, 8), (2, 2))]
CUBIC_LENS_R = [(Y, (12, 8), (8, 7), (8, 3), (12, 2)), (CY, (12, 2), (12, 8))]
A4, B4 = rect(2, 2, 6, 6), rect(8, 2, 12, 6, cols=(Y, CY, M, Y))
SQ = rect(2, 2, 10, 10)
SQ2 = rect(2, 2, 10, 10, cols=(Y, CY, M, Y))

# family -> [(name, contours, w, h, scale, px_range)]; "auto" as scale: autoframe (the one non-lattice framing)
TABLE = {
    "lattice_ties": [
        ("two_squares", [A4, B4], 14, 8, 1, 4),
        ("two_squares_swapped", [B4, A4], 14, 8, 1, 4),
        ("half_lattice_squares", [rect(2.5, 2.5, 5.5, 5.5), rect(8.5, 2.5, 11.5, 5.5, cols=(M, Y, CY, M))], 14, 8, 1, 4),
        ("four_squares", grid(2, 2, 4, 8), 16, 16, 1, 4),
        ("ring", [rect(2, 2, 14, 14), rect(6, 6, 10, 10, flip=True, cols=(Y, M, CY, Y))], 16, 16, 1, 4),
        ("ring_hole_first", [rect(6, 6, 10, 10, flip=True, cols=(Y, M, CY, Y)), rect(2, 2, 14, 14)], 16, 16, 1, 4),
        ("diamond", [DIAMOND], 16, 16, 1, 4),
        ("quad_sides", [QUAD_SIDES], 14, 14, 1, 4),
        ("cubic_sides", [CUBIC_SIDES], 14, 14, 1, 4),
        ("quad_pair", [QUAD_LENS_L, QUAD_LENS_R], 14, 10, 1, 4),
        ("cubic_pair", [CUBIC_LENS_R, CUBIC_LENS_L], 14, 10, 1, 4),
        ("six_squares", grid(3, 2, 2, 4), 28, 20, 2, 4),
        ("grid_6x6", grid(6, 6, 2, 5), 64, 64, 2, 4),                        # 36 contours, 144 edges
    ],
    "on_outline": [
        ("square", [SQ], 12, 12, 1, 4),
        ("diamond", [DIAMOND], 16, 16, 1, 4),
        ("quad_through_lattice", [[(CY, (2, 2), (6, 10), (10, 2)), (M, (10, 2), (2, 2))]], 12, 8, 1, 4),
        ("ring_half_scale", [rect(2, 2, 14, 14), rect(6, 6, 10, 10, flip=True, cols=(Y, M, CY, Y))], 32, 32, 2, 4),
    ],
    "coincident": [
        ("duplicate", [SQ, SQ], 12, 12, 1, 4),
        ("duplicate_recolour", [SQ, SQ2], 12, 12, 1, 4),
        ("reversed", [SQ, rect(2, 2, 10, 10, flip=True)], 12, 12, 1, 4),
        ("shared_edge", [rect(2, 2, 7, 10), rect(7, 2, 12, 10, cols=(Y, CY, M, Y))], 14, 12, 1, 4),
        ("shared_vertex", [rect(2, 2, 7, 7), rect(7, 7, 12, 12, cols=(Y, CY, M, Y))], 14, 14, 1, 4),
        ("six_contours", [A4, B4, rect(2, 2, 6, 6, cols=(M, Y, CY, M)), B4, rect(2, 2, 6, 6, flip=True), rect(8, 2, 12, 6)], 14, 8, 1, 4),
        ("duplicate_offgrid", [SQ, SQ], 13, 11, "auto", 3),
    ],
    "degenerate_edges": [
        ("zero_line", [[(CY, (2, 2), (10, 2)), (M, (10, 2), (10, 2)), (Y, (10, 2), (6, 9)), (CY, (6, 9), (2, 2))]], 12, 12, 1, 4),
        ("quad_ctrl_on_end", [[(CY, (2, 2), (2, 2), (10, 2)), (M, (10, 2), (6, 9), (6, 9)), (Y, (6, 9), (2, 2))]], 12, 12, 1, 4),
        ("quad_collinear", [[(CY, (2, 2), (6, 2), (10, 2)), (M, (10, 2), (9, 3.75), (6, 9)), (Y, (6, 9), (4, 5.5), (2, 2))]], 12, 12, 1, 4),
        ("quad_collinear_beyond", [[(CY, (2, 2), (14, 2), (10, 2)), (M, (10, 2), (6, 9)), (Y, (6, 9), (2, 2))]], 16, 12, 1, 4),
        ("cubic_p1_on_p0", [[(CY, (2, 2), (2, 2), (8, 0), (10, 2)), (M, (10, 2), (6, 9)), (Y, (6, 9), (2, 2))]], 12, 12, 1, 4),
        ("cubic_p2_on_p3", [[(CY, (2, 2), (4, 0), (10, 2), (10, 2)), (M, (10, 2), (6, 9)), (Y, (6, 9), (2, 2))]], 12, 12, 1, 4),
        ("cubic_ends_coincide", [[(CY, (2, 2), (2, 2), (10, 2), (10, 2)), (M, (10, 2), (10, 2), (8, 6), (6, 9)), (Y, (6, 9), (3, 4), (2, 2), (2, 2))]], 12, 12, 1, 4),
        ("cubic_is_line", [[(CY, (2, 2), (4, 2), (8, 2), (10, 2)), (M, (10, 2), (6, 9)), (Y, (6, 9), (2, 2))]], 12, 12, 1, 4),
        ("cubic_all_same", [[(CY, (2, 2), (10, 2)), (W, (10, 2), (10, 2), (10, 2), (10, 2)), (M, (10, 2), (6, 9)), (Y, (6, 9), (2, 2))]], 12, 12, 1, 4),
        ("cubic_cusp", [[(CY, (2, 2), (12, 10), (2, 10), (12, 2)), (M, (12, 2), (2, 2))]], 14, 12, 1, 4),
        ("cubic_loop", [[(W, (6, 2), (16, 12), (-4, 12), (6, 2))]], 12, 12, 1, 4),
        ("two_edge", [[(CY, (2, 6), (6, 0), (10, 6)), (M, (10, 6), (6, 12), (2, 6))]], 12, 12, 1, 4),
        ("two_line_zero_area", [[(CY, (2, 6), (10, 6)), (M, (10, 6), (2, 6))]], 12, 12, 1, 4),
        ("quad_fold_back", [[(CY, (2, 2), (10, 2), (2, 2)), (M, (2, 2), (6, 9)), (Y, (6, 9), (2, 2))]], 12, 12, 1, 4),
    ],
    "sparse_colours": [
        ("black_edge", [rect(2, 2, 10, 10, cols=(CY, K, Y, M))], 12, 12, 1, 4),
        ("all_black", [rect(2, 2, 10, 10, cols=(K, K, K, K))], 12, 12, 1, 4),
        ("single_channels", [rect(2, 2, 10, 10, cols=(R, G, B, R))], 12, 12, 1, 4),
        ("all_cyan", [rect(2, 2, 10, 10, cols=(CY, CY, CY, CY))], 12, 12, 1, 4),
        ("all_white", [rect(2, 2, 10, 10, cols=(W, W, W, W)), rect(4, 4, 8, 8, flip=True, cols=(W, W, W, W))], 12, 12, 1, 4),
        ("contour_without_red", [SQ, rect(4, 4, 8, 8, flip=True, cols=(CY, CY, CY, CY))], 12, 12, 1, 4),
        ("red_only_curves", [[(R, (2, 6), (6, 0), (10, 6)), (R, (10, 6), (6, 12), (2, 6))]], 12, 12, 1, 4),
    ],
    "scanline_hits": [
        ("square", [SQ], 12, 12, 1, 4),
        ("diamond", [DIAMOND], 16, 16, 1, 4),
        ("quad_extremum", [[(CY, (2, 6), (6, 0), (10, 6)), (M, (10, 6), (6, 12), (2, 6))]], 12, 12, 1, 4),
        ("cubic_extremum", [[(CY, (2, 4), (2, 12), (10, 12), (10, 4)), (M, (10, 4), (2, 4))]], 12, 12, 1, 4),
        ("peaks", [poly([(2, 2), (12, 2), (12, 8), (9, 5), (7, 8), (5, 5), (2, 8)])], 14, 10, 1, 4),
        ("ring_half_scale", [rect(2, 2, 14, 14), rect(6, 6, 10, 10, flip=True, cols=(Y, M, CY, Y))], 32, 32, 2, 4),
    ],
    "slivers": [
        ("thin_rect", [rect(2, 6, 10, 6+1e-9)], 12, 12, 1, 4),
        ("subtexel", [rect(6.25, 6.25, 6.5, 6.5)], 12, 12, 1, 4),
        ("half_texel_bar", [rect(2, 6, 10, 6.5)], 12, 12, 1, 4),
        ("bar_thinner_than_range", [rect(2, 5.5, 10, 6.25)], 12, 12, 1, 4),
        ("thin_column_and_square", [rect(2, 2, 2.5, 10), rect(5, 4, 9, 8, cols=(Y, CY, M, Y))], 12, 12, 1, 4),
    ],
}

# What check_premise() demands at least, per case at its own size, as the oracle counts it (tools/make_golden_geometry.py --premises prints the table):
# lattice_ties: texel centres whose smallest |distance| is shared, exactly, by two edges that are not neighbours; on_outline: texel centres at distance
# exactly 0; coincident: vertices two contours share; scanline_hits: texel-centre rows through a vertex or a curve's y extremum; slivers: a contour box thinner than one texel; the rest: 1.
MIN_COUNT = {}


def _shape(contours):
    return FlatShape.from_contours(contours)


def _fit_scale(nw, nh, ns, w, h):
    """The largest power-of-two multiple of the case's own scale at which its own bitmap still fits into w x h (never below the case's scale)."""
    s = ns
    while nw*(2*s/ns) <= w and nh*(2*s/ns) <= h:
        s *= 2
    return s


def family_cases(family, seed=0, w=None, h=None):
    """The cases of one family. seed 0: the table as it stands; other seeds: each case after jitter(). w, h: every case re-framed into that bitmap at a
    dyadic scale (cases whose own bitmap is larger are left out)."""
    out = []
    for k, (name, contours, nw, nh, ns, pr) in enumerate(TABLE[family]):
        rng = np.random.default_rng([FAMILIES.index(family), seed, k])
        full = "%s/%s" % (family, name)
        bw, bh = (nw, nh) if w is None else (w, h)
        if bw < nw or bh < nh:
            continue
        shape = _shape(contours)
        if ns == "auto":
            xf = autoframe(shape.bounds(), bw, bh, pr)
        else:
            xf = lattice_xf(ns if family == "slivers" else _fit_scale(nw, nh, ns, bw, bh), pr)   # a sliver magnified is none
        y_down = bool((k+seed) & 1)
        if seed:
            shape, xf = jitter(shape, xf, rng)
            full += "~%d" % seed
        if w is not None:
            full += "@%dx%d" % (bw, bh)
        out.append(Case(full, shape, bw, bh, xf, y_down))
    return out


def cases(families=FAMILIES, seeds=(0,), w=None, h=None):
    return [c for f in families for sd in seeds for c in family_cases(f, sd, w, h)]


def base_name(case):
    return case.name.split("~")[0].split("@")[0]


def bit_exact(cs):
    return [c for c in cs if base_name(c) not in SIGN_NOISE]


def contours_of(shape):
    """[[(color, p0, ..), ..], ..] of a FlatShape: the form FlatShape.from_contours takes."""
    out = []
    for c in range(shape.n_contours):
        e0, e1 = int(shape.contour_offsets[c]), int(shape.contour_offsets[c+1])
        out.append([(int(shape.colors[e]),)+tuple((float(shape.points[e, 2*i]), float(shape.points[e, 2*i+1])) for i in range(int(shape.types[e])+1))
                    for e in range(e0, e1)])
    return out


def strip_colours(shape):
    """All edges WHITE: the input of shape preparation."""
    return FlatShape(shape.contour_offsets.copy(), shape.points.copy(), shape.types.copy(), np.full_like(shape.colors, W), shape.inverse_y)


def jitter(shape, xf, rng):
    """Lattice-preserving moves: every one is exact in fp64 for dyadic coordinates, so a premise holds after it as before. An integer translation and a
    power-of-two scale of the outline, each undone by the transform; a permutation of the contours; a permutation of the colour channels; reversed contours."""
    cs = contours_of(shape)
    xf = np.array(xf, np.float64)
    dx, dy = (float(v) for v in rng.integers(-3, 4, 2))
    k = 2.**int(rng.integers(-2, 3))
    cs = [[(e[0],)+tuple(((x+dx)*k, (y+dy)*k) for x, y in e[1:]) for e in c] for c in cs]
    xf = np.array([xf[0]/k, xf[1]/k, (xf[2]-dx)*k, (xf[3]-dy)*k, xf[4]*k, xf[5]*k])
    cs = [cs[i] for i in rng.permutation(len(cs))]
    perm = rng.permutation(3)
    recolour = lambda c: sum(1 << int(perm[b]) for b in range(3) if c >> b & 1)
    cs = [[(recolour(e[0]),)+e[1:] for e in c] for c in cs]
    if rng.integers(0, 2):
        cs = [[(e[0],)+e[:0:-1] for e in c[::-1]] for c in cs]
    return FlatShape.from_contours(cs, shape.inverse_y), xf


def texel_points(case):
    """(h*w, 2) float64: the shape-space point of every texel centre, as Projection::unproject computes it (coordinate / scale - translate)."""
    xs = (np.arange(case.w)+.5)/case.xf[0]-case.xf[2]
    ys = (np.arange(case.h)+.5)/case.xf[1]-case.xf[3]
    return np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)


def edge_distances(oracle, shape, pts):
    """(len(pts), E) float64: |signed distance| of every edge at every point, from the oracle's per-edge signedDistance."""
    fn = oracle.lib.orc_signed_distance
    out = np.zeros((len(pts), shape.n_edges))
    res = (C.c_double*3)()
    rows = [(int(shape.types[e]), np.ascontiguousarray(shape.points[e]).ctypes.data_as(C.POINTER(C.c_double))) for e in range(shape.n_edges)]
    keep = shape.points                                             # the pointers above point into it
    for i, (x, y) in enumerate(pts.tolist()):
        for e, (t, p) in enumerate(rows):
            fn(t, p, x, y, res)
            out[i, e] = abs(res[0])
    del keep
    return out


def _adjacent(shape):
    """(E, E) bool: the same edge, or neighbours in their contour's cycle."""
    n = shape.n_edges
    adj = np.eye(n, dtype=bool)
    for c in range(shape.n_contours):
        e0, e1 = int(shape.contour_offsets[c]), int(shape.contour_offsets[c+1])
        for e in range(e0, e1):
            nxt = e0+(e+1-e0) % (e1-e0)
            adj[e, nxt] = adj[nxt, e] = True
    return adj


def tie_texels(oracle, case, pts=None):
    """Indices of the points (default: texel centres) whose smallest per-edge |distance| is attained, exactly, by two edges that are not neighbours."""
    pts = texel_points(case) if pts is None else pts
    d = edge_distances(oracle, case.shape, pts)
    adj = _adjacent(case.shape)
    hit = []
    for i in range(len(pts)):
        m = np.flatnonzero(d[i] == d[i].min())
        if len(m) >= 2 and not adj[np.ix_(m, m)].all():
            hit.append(i)
    return np.array(hit, int)


def tie_points(case):
    """Query points for the cooperative-merge checks (psdf_cooperative, shape_distance): the texel centres plus every vertex."""
    return np.vstack([texel_points(case), case.shape.points[:, 0:2]])


def zero_texels(oracle, case):
    d = edge_distances(oracle, case.shape, texel_points(case))
    return np.flatnonzero(d.min(axis=1) == 0)


def shared_vertices(shape):
    """Start points that occur in two different contours (exactly equal coordinates)."""
    seen = {}
    for c in range(shape.n_contours):
        for e in range(int(shape.contour_offsets[c]), int(shape.contour_offsets[c+1])):
            seen.setdefault((float(shape.points[e, 0]), float(shape.points[e, 1])), set()).add(c)
    return sum(1 for v in seen.values() if len(v) > 1)


def _cps(shape, e):
    return [shape.points[e, 2*i:2*i+2] for i in range(int(shape.types[e])+1)]


def degeneracies(shape):
    """Names of the degenerate forms present: the branches of the solvers and of the direction fall-backs that an ordinary outline never takes."""
    found = set()
    for c in range(shape.n_contours):
        n = int(shape.contour_offsets[c+1]-shape.contour_offsets[c])
        if 0 < n <= 2:
            found.add("contour_of_%d" % n)
    for e in range(shape.n_edges):
        p = _cps(shape, e)
        if all((q == p[0]).all() for q in p[1:]):
            found.add("zero_length")
            continue
        if (p[0] == p[-1]).all():
            found.add("closed_edge")
        if len(p) > 2:
            if (p[1] == p[0]).all() or (p[-2] == p[-1]).all():
                found.add("control_on_end")
            d = p[-1]-p[0]
            if all(float(d[0]*(q-p[0])[1]-d[1]*(q-p[0])[0]) == 0 for q in p[1:-1]):
                found.add("collinear")
    return found


def colour_census(shape):
    """(channels no edge of the glyph has, contours lacking a channel, edges coloured BLACK or with a single channel, contours of two or more edges
    that all carry one colour). A corner-alternating CYAN / MAGENTA / YELLOW colouring has none of the four."""
    glyph = lacking = odd = uniform = 0
    for c in range(shape.n_contours):
        cols = [int(shape.colors[e]) for e in range(int(shape.contour_offsets[c]), int(shape.contour_offsets[c+1]))]
        m = 0
        for v in cols:
            m |= v
        glyph |= m
        lacking += bool(cols) and m != 7
        odd += sum(v in (K, R, G, B) for v in cols)
        uniform += len(cols) >= 2 and len(set(cols)) == 1
    return 7 & ~glyph, lacking, odd, uniform


def scanline_rows(case):
    """Texel-centre rows whose scanline passes exactly through an edge's end point or through the y extremum of a quadratic or cubic edge."""
    s = case.shape
    ys = set()
    for e in range(s.n_edges):
        p = _cps(s, e)
        ys.update((float(p[0][1]), float(p[-1][1])))
        if len(p) == 3:
            den = float(p[0][1]-2*p[1][1]+p[2][1])
            if den != 0:
                t = float(p[0][1]-p[1][1])/den
                if 0 < t < 1:
                    ys.add(float((1-t)*(1-t)*p[0][1]+2*(1-t)*t*p[1][1]+t*t*p[2][1]))
        elif len(p) == 4:                                            # dy/dt = 0: a quadratic in t
            a = float(-p[0][1]+3*p[1][1]-3*p[2][1]+p[3][1])
            b = float(2*(p[0][1]-2*p[1][1]+p[2][1]))
            c = float(p[1][1]-p[0][1])
            roots = []
            if a != 0 and b*b-4*a*c >= 0:
                r = float(np.sqrt(b*b-4*a*c))
                roots = [(-b+r)/(2*a), (-b-r)/(2*a)]
            elif a == 0 and b != 0:
                roots = [-c/b]
            for t in roots:
                if 0 < t < 1:
                    ys.add(float((1-t)**3*p[0][1]+3*(1-t)**2*t*p[1][1]+3*(1-t)*t*t*p[2][1]+t**3*p[3][1]))
    rows = (np.arange(case.h)+.5)/case.xf[1]-case.xf[3]
    return [int(r) for r in range(case.h) if float(rows[r]) in ys]


def thinnest_feature(case):
    """The smaller side of the narrowest contour box, in texels."""
    s = case.shape
    best = np.inf
    for c in range(s.n_contours):
        pts = np.concatenate([_cps(s, e) for e in range(int(s.contour_offsets[c]), int(s.contour_offsets[c+1]))])
        if len(pts):
            ext = pts.max(axis=0)-pts.min(axis=0)
            best = min(best, float(ext[0]*abs(case.xf[0])), float(ext[1]*abs(case.xf[1])))
    return best


def premise_count(case, oracle):
    """The number check_premise() compares with MIN_COUNT: what the family counts, at this case's framing."""
    fam = case.name.split("/")[0]
    if fam == "lattice_ties":
        return len(tie_texels(oracle, case))
    if fam == "on_outline":
        return len(zero_texels(oracle, case))
    if fam == "coincident":
        return shared_vertices(case.shape)
    if fam == "degenerate_edges":
        return len(degeneracies(case.shape))
    if fam == "sparse_colours":
        missing, lacking, odd, uniform = colour_census(case.shape)
        return int(missing != 0)+lacking+odd+uniform
    if fam == "scanline_hits":
        return len(scanline_rows(case))
    if fam == "slivers":
        return int(thinnest_feature(case) < 1)
    raise AssertionError("unknown family %r" % fam)


def check_premise(case, oracle):
    """Assert what makes `case` a member of its family. An ordinary synth glyph under autoframe fails every one of them."""
    need = MIN_COUNT.get(base_name(case), 1)
    got = premise_count(case, oracle)
    assert need >= 1 and got >= need, "%s: premise: %d, the case table states at least %d" % (case.name, got, need)


MIN_COUNT.update({
    "lattice_ties/two_squares": 10, "lattice_ties/two_squares_swapped": 10, "lattice_ties/half_lattice_squares": 10, "lattice_ties/four_squares": 35,
    "lattice_ties/ring": 21, "lattice_ties/ring_hole_first": 21, "lattice_ties/diamond": 1, "lattice_ties/quad_sides": 1, "lattice_ties/cubic_sides": 1,
    "lattice_ties/quad_pair": 6, "lattice_ties/cubic_pair": 4, "lattice_ties/six_squares": 72, "lattice_ties/grid_6x6": 651,
    "on_outline/square": 32, "on_outline/diamond": 24, "on_outline/quad_through_lattice": 11, "on_outline/ring_half_scale": 128,
    "coincident/duplicate": 4, "coincident/duplicate_recolour": 4, "coincident/reversed": 4, "coincident/shared_edge": 2, "coincident/shared_vertex": 1,
    "coincident/six_contours": 8, "coincident/duplicate_offgrid": 4,
    "scanline_hits/square": 2, "scanline_hits/diamond": 3, "scanline_hits/quad_extremum": 3, "scanline_hits/cubic_extremum": 2, "scanline_hits/peaks": 3,
    "scanline_hits/ring_half_scale": 4,
})

EC_PAIRS = [(m, d) for m in range(4) for d in range(3)]
ALWAYS_CHECK = 2                                                   # DistanceCheckMode::ALWAYS_CHECK_DISTANCE


def settings():
    """(key, kwargs) of every generate call the reference comparison makes: Y up and down, both combiners, sdf / psdf, msdf / mtsdf under all twelve
    correction settings."""
    for yd in (False, True):
        for ov in (True, False):
            for mode in (1, 2, 3, 4):
                for ec, dc in (EC_PAIRS if mode >= 3 else [(0, 0)]):
                    yield "m%d o%d y%d ec%d/%d" % (mode, ov, yd, ec, dc), dict(mode=mode, overlap=ov, y_down=yd, ec_mode=ec, ec_dist=dc)


def generate(lib, case, mode, **kw):
    """(values, stencil) of one generate call of Oracle / Ref / Emu-like `lib`."""
    st = np.zeros((case.h, case.w), np.uint8) if mode >= 3 else None
    return lib.generate(case.shape, mode, case.w, case.h, case.xf, stencil=st, **kw), st


def differing(a, b):
    """Flat indices where two float32 arrays differ in their bits (NaN payloads and signs of zero included)."""
    return np.flatnonzero(np.ascontiguousarray(a, np.float32).view(np.uint32).ravel() != np.ascontiguousarray(b, np.float32).view(np.uint32).ravel())


def departures(literal, exact, case):
    """{setting key: {"at": flat value indices, "literal": bits, "exact": bits, "stencil_at": flat texel indices, "stencil_literal", "stencil_exact"}} for
    every setting under which the reference with its cached distance queries (`literal`) and with uncached ones (`exact`) give different output."""
    out = {}
    for key, kw in settings():
        a, sa = generate(literal, case, **kw)
        b, sb = generate(exact, case, **kw)
        at = differing(a, b)
        st = np.flatnonzero(sa.ravel() != sb.ravel()) if sa is not None else np.zeros(0, int)
        if len(at) or len(st):
            out[key] = {"at": at.tolist(), "literal": a.view(np.uint32).ravel()[at].tolist(), "exact": b.view(np.uint32).ravel()[at].tolist(),
                        "stencil_at": st.tolist(), "stencil_literal": sa.ravel()[st].tolist() if len(st) else [],
                        "stencil_exact": sb.ravel()[st].tolist() if len(st) else []}
    return out


def reference_cases():
    """The cases the reference comparison and its fixture cover: every case at its own size, and every case re-framed into each of BIG_SIZES."""
    return cases()+[c for w, h in BIG_SIZES for c in cases(w=w, h=h)]
