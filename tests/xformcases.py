"""Framings other than autoframe's for the parity tests (test_xform_cases.py on the CPU, test_gpu_transforms.py on the GPU, fuzzlib's framing=):
mirrored and anisotropic projections, zooms in and out, glyphs off the tile, inverted / huge / tiny / asymmetric distance ranges, scales whose
significand is all ones (the kernels' non-divExact texel path), far-off shape coordinates, and bitmaps narrower than the 8x8 tile.

A case is (name, shape, w, h, xf, y_down) with xf = (sx, sy, tx, ty, range_lower, range_upper) as autoframe() returns it. Every family states
its premise in check_premise(), so that an edit which turns a family back into the autoframe case fails there instead of passing quietly."""
import math
from collections import namedtuple

import numpy as np

from msdfgen_amd import synth
from msdfgen_amd.shape import FlatShape, autoframe

Case = namedtuple("Case", "name shape w h xf y_down")

MIRRORS = ("mirror_x", "mirror_y", "mirror_xy")
FAMILIES = MIRRORS+("aniso", "zoom_in", "zoom_out", "off_tile", "neg_range", "huge_range", "tiny_range", "asym_range", "nondivsafe", "far_coords",
                    "tiny_bitmaps")
TINY_SIZES = ((1, 1), (1, 9), (9, 1), (2, 2), (3, 7), (7, 3), (8, 1), (1, 64), (65, 2), (17, 9))


def div_safe(b):
    """divSafe (msdf_device.hpp) in numpy: |b| in (1e-100, 1e100) and a significand that is not all ones."""
    m = abs(float(b))
    if not (1e-100 < m < 1e100):
        return False
    return float(np.frexp(m)[0]) != 1-2.0**-53


def projected_bounds(shape, xf):
    """(x0, y0, x1, y1): the control-point box of `shape` in texel units (before any Y flip of the output)."""
    l, b, r, t = shape.bounds()
    xs = sorted((xf[0]*(l+xf[2]), xf[0]*(r+xf[2])))
    ys = sorted((xf[1]*(b+xf[3]), xf[1]*(t+xf[3])))
    return xs[0], ys[0], xs[1], ys[1]


def base_shape(rng):
    """Lines / quadratics / cubics with holes, a CJK-like many-contour glyph, or overlapping blobs."""
    sd = int(rng.integers(0, 2**31))
    kind = int(rng.integers(0, 3))
    if kind == 0:
        s = synth.random_shape(sd, n_contours=int(rng.integers(1, 4)), kinds=(1, 2, 3), holes=True)
    elif kind == 1:
        s = synth.cjk_like_shape(sd)
    else:
        s = synth.random_shape(sd, n_contours=int(rng.integers(3, 7)), kinds=(1, 2, 3), spread=.25, holes=bool(sd & 1))
    s.inverse_y = bool(rng.integers(0, 2))
    return s


def _centred(sx, sy, bounds, w, h):
    l, b, r, t = bounds
    return .5*w/sx-.5*(l+r), .5*h/sy-.5*(b+t)


def _offset(shape, ox, oy):
    """The shape moved by (ox, oy): only the control points an edge uses."""
    pts = shape.points.copy()
    for k in range(4):
        m = shape.types >= max(k, 1)
        pts[m, 2*k] += ox
        pts[m, 2*k+1] += oy
    return FlatShape(shape.contour_offsets.copy(), pts, shape.types.copy(), shape.colors.copy(), shape.inverse_y)


def frame(family, shape, w, h, rng, variant=0):
    """(shape, xf) of `family` for `shape` in a w x h bitmap; far_coords returns a moved copy of the shape. variant picks the sub-form
    (e.g. the ratio of aniso, near or far for off_tile) where a family has several; rng draws the rest."""
    bounds = shape.bounds()
    pr = min(float(rng.choice([2., 3., 4.])), .45*min(w, h))
    xf = autoframe(bounds, w, h, pr)
    s = xf[0]
    l, b, r, t = bounds
    if family in MIRRORS:
        if family in ("mirror_x", "mirror_xy"):
            xf[0], xf[2] = -s, xf[2]-w/s                    # X' = w - X
        if family in ("mirror_y", "mirror_xy"):
            xf[1], xf[3] = -s, xf[3]-h/s                    # Y' = h - Y
    elif family == "aniso":
        fx, fy = w-pr, h-pr
        dx, dy = max(r-l, 1e-9), max(t-b, 1e-9)
        if variant % 2 == 0:                                # sx/sy = 8: a tile spans 8 times more shape space in y than in x (its radius is hy's);
            sy = max(fy, 32.)/dy                            # the glyph is at least four tiles tall and 8 times wider than that, past the
            sx = 8*sy                                       # bitmap: the cull has tiles far from most edges
        else:                                               # sx/sy = 1/8
            sx = max(fx, 32.)/dx
            sy = 8*sx
        tx, ty = _centred(sx, sy, bounds, w, h)
        lo = -.5*pr/max(sx, sy)
        xf = np.array([sx, sy, tx, ty, lo, -lo])
    elif family == "zoom_in":
        k = 2.**rng.uniform(2, 6)                           # x4 .. x64
        s = s*k
        cx, cy = rng.uniform(l, r), rng.uniform(b, t)       # a point of the box lands at a random texel position
        u, v = rng.uniform(0, 1, 2)
        lo = -.5*pr/s
        xf = np.array([s, s, u*w/s-cx, v*h/s-cy, lo, -lo])
    elif family == "zoom_out":
        span = rng.uniform(1.5, 4.)                         # the glyph covers a few texels
        s = span/max(r-l, t-b, 1e-9)
        u, v = rng.uniform(.25, .75, 2)
        lo = -.5*pr/s
        xf = np.array([s, s, u*w/s-.5*(l+r), v*h/s-.5*(b+t), lo, -lo])
    elif family == "off_tile":
        gap = rng.uniform(.6, 3.) if variant % 2 == 0 else 10.**rng.uniform(3, 5)   # texels between the box and the tile: near, far
        side = int(rng.integers(0, 4))
        tx, ty = _centred(s, s, bounds, w, h)
        if side == 0:
            tx = -gap/s-r                                   # box right of x = -gap
        elif side == 1:
            tx = (w+gap)/s-l
        elif side == 2:
            ty = -gap/s-t
        else:
            ty = (h+gap)/s-b
        xf[2], xf[3] = tx, ty
    elif family == "neg_range":
        xf[4], xf[5] = xf[5], xf[4]*rng.uniform(.5, 1.5)    # lower > upper: a negative mapScale
    elif family == "huge_range":
        width = rng.uniform(1.5, 20.)*max(w, h)             # wider than the tile, in texels
        xf[4], xf[5] = -.5*width/s, .5*width/s
    elif family == "tiny_range":
        xf[4], xf[5] = -.5e-3/s, .5e-3/s                    # 1e-3 texels
    elif family == "asym_range":
        a, c = rng.uniform(.2, 1.), rng.uniform(2., 6.)
        xf[4], xf[5] = (-a/s, c/s) if variant % 2 == 0 else (-c/s, a/s)
    elif family == "nondivsafe":
        ones = np.nextafter(2.**math.floor(math.log2(s)), 0.)   # all-ones significand, <= s: still fits
        sx, sy = (ones, ones) if variant % 3 == 0 else ((ones, s) if variant % 3 == 1 else (s, ones))
        tx, ty = _centred(sx, sy, bounds, w, h)
        xf[:4] = sx, sy, tx, ty
    elif family == "far_coords":
        o = 10.**rng.uniform(4, 7)*rng.choice([-1., 1.], 2)
        shape = _offset(shape, o[0], o[1])
        bounds = shape.bounds()
        l, b, r, t = bounds
        if variant % 2 == 0:                                # x1: the autoframe scale with a sub-texel shift
            xf = autoframe(bounds, w, h, pr)
            xf[2] += rng.uniform(.1, .4)/xf[0]
            xf[3] -= rng.uniform(.1, .4)/xf[1]
        else:                                               # x50, anchored like zoom_in
            s = s*50
            cx, cy = rng.uniform(l, r), rng.uniform(b, t)
            lo = -.5*pr/s
            xf = np.array([s, s, .5*w/s-cx, .5*h/s-cy, lo, -lo])
    elif family == "tiny_bitmaps":
        xf = autoframe(bounds, w, h, min(2., .5*min(w, h)))
    else:
        raise ValueError("unknown framing family %r" % family)
    return shape, np.asarray(xf, np.float64)


def family_cases(family, seed, w=None, h=None):
    """The cases of one family for one seed. w, h: the bitmap size (None: drawn); tiny_bitmaps always walks TINY_SIZES."""
    rng = np.random.default_rng([FAMILIES.index(family), seed])
    out = []
    if family == "tiny_bitmaps":
        for k, (tw, th) in enumerate(TINY_SIZES):
            s = base_shape(rng)
            s2, xf = frame(family, s, tw, th, rng)
            out.append(Case("%s/%dx%d/%d" % (family, tw, th, seed), s2, tw, th, xf, bool(rng.integers(0, 2))))
        return out
    n = 4 if family in MIRRORS else 2
    for k in range(n):
        bw = int(w if w is not None else rng.integers(9, 49))
        bh = int(h if h is not None else rng.integers(9, 49))
        s = base_shape(rng)
        if family in MIRRORS:                               # inverse_y x y_down
            s.inverse_y, yd = bool(k & 1), bool(k & 2)
        else:
            yd = bool(rng.integers(0, 2))
        s2, xf = frame(family, s, bw, bh, rng, variant=seed*n+k)
        out.append(Case("%s/%d.%d" % (family, seed, k), s2, bw, bh, xf, yd))
    return out


def cases(families=FAMILIES, seeds=(0,), w=None, h=None):
    return [c for f in families for sd in seeds for c in family_cases(f, sd, w, h)]


def check_premise(case, oracle=None):
    """Assert what makes `case` a member of its family rather than an autoframed glyph. With `oracle`, also the premises that need distances."""
    fam = case.name.split("/")[0]
    xf, w, h = case.xf, case.w, case.h
    x0, y0, x1, y1 = projected_bounds(case.shape, xf)
    inside = x0 >= -1e-9 and y0 >= -1e-9 and x1 <= w+1e-9 and y1 <= h+1e-9
    what = "%s: premise" % case.name
    assert np.isfinite(xf).all() and xf[0] != 0 and xf[1] != 0 and xf[4] != xf[5], what
    if fam in MIRRORS:
        assert (xf[0] < 0) == (fam != "mirror_y") and (xf[1] < 0) == (fam != "mirror_x") and inside, what
    elif fam == "aniso":
        ratio = abs(xf[0]/xf[1])
        assert max(ratio, 1/ratio) >= 8*(1-1e-12), what
    elif fam == "zoom_in":
        assert not inside and x1 > 0 and y1 > 0 and x0 < w and y0 < h, what       # partly outside the tile, and reaching into it
    elif fam == "zoom_out":
        assert x1-x0 <= 4 and y1-y0 <= 4 and inside, what
    elif fam == "off_tile":
        assert x1 < .5 or x0 > w-.5 or y1 < .5 or y0 > h-.5, what                # no texel centre inside the box
    elif fam == "neg_range":
        assert xf[4] > xf[5], what
    elif fam == "huge_range":
        assert (xf[5]-xf[4])*min(abs(xf[0]), abs(xf[1])) > max(w, h), what
    elif fam == "tiny_range":
        assert 0 < (xf[5]-xf[4])*max(abs(xf[0]), abs(xf[1])) <= 1.5e-3, what
    elif fam == "asym_range":
        assert xf[4] < xf[5] and abs(xf[4]+xf[5]) >= .2*(xf[5]-xf[4]), what
    elif fam == "nondivsafe":
        assert not (div_safe(xf[0]) and div_safe(xf[1])), what
    elif fam == "far_coords":
        pts = case.shape.points
        used = np.concatenate([pts[case.shape.types >= max(k, 1), 2*k:2*k+2] for k in range(4)])
        assert np.abs(used).min() >= 5e3, what
        auto = autoframe(case.shape.bounds(), w, h, 2*abs(xf[4])*xf[0])
        assert not np.array_equal(xf[:4], auto[:4]), what
    elif fam == "tiny_bitmaps":
        assert (w, h) in TINY_SIZES and (min(w, h) < 8 or w % 8 == 1 or h % 8 == 1), what
    else:
        raise AssertionError("unknown family %r" % fam)
    if oracle is not None and fam in ("zoom_in", "off_tile"):
        sdf = oracle.generate(case.shape, 1, w, h, xf, y_down=case.y_down)
        d = (sdf[..., 0].astype(np.float64)-.5)*(xf[5]-xf[4])*abs(xf[0])            # signed distance in texels (symmetric range)
        if fam == "zoom_in":
            assert (np.abs(d) > (xf[5]-xf[4])*abs(xf[0])).any(), what+": no texel beyond the range"
        else:
            assert (np.abs(d) > .5).all(), what+": a texel on the shape"
