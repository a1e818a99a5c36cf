"""The GPU side of tests/test_gpu_devmath.py, run by it as a child process under a time limit: every device call the test needs, results into one .npz.

    python tests/devmath_gpu_child.py OUT.npz

The arithmetic primitives go through tests/devmath (ctypes only); the inputs are those of tests/devmathcases.py, which the parent builds again to compare.
Before them, the one product call of the file: the start-point glyphs through GlyphBatch.generate (tiles_<mode>)."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import devmathcases as D  # noqa: E402
from devmath import DevMath  # noqa: E402


def kats():
    return np.load(os.path.join(HERE, "golden", "kats.npz"))


def kat_edges(z):
    """The 3 x 200 signedDistance rows of kats.npz as one (types, points, origins) call."""
    types = np.repeat(np.array([1, 2, 3], np.int32), 200)
    return types, np.concatenate([z["sd%d_pts" % t] for t in (1, 2, 3)]), np.concatenate([z["sd%d_org" % t] for t in (1, 2, 3)])


def kat_normed_rows(z):
    """The rows of cubic_coef that solveCubic hands to solveCubicNormed (a != 0 and |b/a| < 1e6, equation-solver.cpp:63-70), normalised as it does."""
    c = z["cubic_coef"]
    with np.errstate(all="ignore"):
        bn = c[:, 1]/c[:, 0]
        normed = (c[:, 0] != 0) & (np.abs(bn) < 1e6)
    idx = np.nonzero(normed)[0]
    return idx, np.stack([bn[idx], c[idx, 2]/c[idx, 0], c[idx, 3]/c[idx, 0]], 1)


MAPPINGS = ((.25, 2.), (1/3., .7), (.125, 4.), (1., .5))          # (scale, translate) of the mapDistance checks


def main(out_path):
    t0 = time.time()
    out = {}
    # The product call first: torch brings its own HIP runtime, and a process has to load that one before any other (msdfgen_amd/lib.py); the harness then
    # shares it, as the product's library does.
    import msdfgen_amd as M
    from msdfgen_amd.shape import ShapeBatch
    M.init(0)
    shapes = D.start_point_glyphs()
    gb = M.GlyphBatch(ShapeBatch.from_shapes(shapes))
    w, h = D.GLYPH_SIZE
    xfs = np.tile(D.GLYPH_XF, (len(shapes), 1))
    for mode in (1, 2, 3, 4):
        out["tiles_%d" % mode] = gb.generate(mode, w, h, xfs).cpu().numpy()
    gb.close()
    t1 = time.time()
    dm = DevMath()
    assert dm.arch().startswith("gfx950"), dm.arch()
    x, _ = D.sqrt_inputs()
    out["sqrt_lean"] = dm.sqrt(x)
    out["sqrt_compiler"] = dm.sqrt(x, compiler=True)
    out["cos_thirds"] = dm.cos_thirds(D.cos_thirds_inputs()[0])
    out["pow_third"] = dm.pow_third(D.pow_third_inputs()[0])
    out["acos"] = dm.acos(D.acos_inputs()[0])
    for name, (a, b) in D.div_inputs().items():
        out["div_safe_"+name], out["div_q_"+name], out["div_ieee_"+name] = dm.div(a, b)
    z = kats()
    out["quad_kat_n"], out["quad_kat_x"] = dm.solve_quadratic(z["cubic_coef"][:, 1:])
    out["quad_n"], out["quad_x"] = dm.solve_quadratic(D.quadratic_inputs())
    _, rows = kat_normed_rows(z)
    out["cubic_kat_n"], out["cubic_kat_x"], out["cubic_kat_trig"] = dm.solve_cubic_normed_pre(*rows.T)
    out["cubic_n"], out["cubic_x"], out["cubic_trig"] = dm.solve_cubic_normed_pre(*D.cubic_inputs().T)
    out["sd"], out["sd_flags"] = dm.signed_distance(*kat_edges(z))
    d = np.concatenate([out["sd"][:, 0], np.concatenate([z["sd%d_out" % t][:, 0] for t in (1, 2, 3)])])
    for k, (scale, translate) in enumerate(MAPPINGS):
        out["map_%d" % k] = dm.map_distance(scale, translate, d)
    out["float_above"] = dm.float_above(D.float_above_inputs())
    out["wave_min"] = dm.wave_min(D.wave_min_inputs()).reshape(-1, 64)
    out["row_min"] = dm.wave_min(D.row_min_inputs(), rows=True).reshape(-1, 64)
    out["row_rank"] = dm.row_rank(D.row_rank_inputs()).reshape(-1, 64)
    np.savez(out_path, **out)
    print("wrote %d arrays; product %.2f s, primitives %.2f s" % (len(out), t1-t0, time.time()-t1))


if __name__ == "__main__":
    main(sys.argv[1])
