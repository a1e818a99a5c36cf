"""The GPU side of tests/test_gpu_ec_roots.py, run by it as a child process under a time limit: every device call the test needs, results into one .npz.

    python tests/ecroots_gpu_child.py OUT.npz

tiles_<w>_<h>_<n>_<y>_<mode>_<check>, stencil_...   GlyphBatch.generate of the twelve fixture glyphs with a stencil buffer (filled with 77 before the call)
single_<w>_<h>_<mode>_<check>, singlest_...         generate_msdf of one glyph alone (k_single_call), stencil through ErrorCorrectionConfig.buffer
shapeless_<i>_<p>                                   field i of shapeless_fields() through msdf_fast_distance_error_correction (p = 0) /
                                                    msdf_fast_edge_error_correction (p = 1)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import eclazycases as E  # noqa: E402
import ecrootscases as R  # noqa: E402
import ecwordscases as W  # noqa: E402
import ecwords_gpu_child as words  # noqa: E402

SIZES = words.SIZES                      # 1x1, 3x5, 8x8, 9x9, 10x17, 23x17
CONFIGS = words.CONFIGS                  # the library default (lazy order); EDGE_PRIORITY + DO_NOT_CHECK; EDGE_PRIORITY + ALWAYS_CHECK (both eager)
SINGLE_CONFIGS = words.SINGLE_CONFIGS
fixture, frames, single_glyph = words.fixture, words.frames, words.single_glyph


def shapeless_fields():
    """The crafted cells (8x8, 9x9), the crafted special-value fields (1x1 to 10x17), the seeded plane-wave fields of this file's cases at 8x8 and 9x9 and
    those of tests/eclazycases.py (16x16, 23x17; one row order: the shapeless entries know none)."""
    from msdfgen_amd.shape import ShapeBatch
    z = np.load(os.path.join(HERE, "golden", "latin.npz"))
    batch = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                       z["colors"].astype(np.int32), z["inverse_y"], [str(n) for n in z["names"]])
    waves = [c for c in R.extra_cases(range(20, 26)) if (c["w"], c["h"]) in R.CRAFTED_SIZES]+[c for c in E.random_cases(batch, z["bounds"]) if c["flip"] == 0]
    return [{"w": c["w"], "h": c["h"], "field": np.ascontiguousarray(c["field"], np.float32)} for c in R.crafted_cases()+W.crafted_cases()+waves]


def main(out_path):
    import torch
    import msdfgen_amd as M
    M.init(0)
    assert M.device_info()["arch"].startswith("gfx950"), M.device_info()
    sub, bounds = fixture()
    gb = M.GlyphBatch(sub)
    out = {}

    def config(mode, dist, buffer=None):
        return M.MSDFGeneratorConfig(True, M.ErrorCorrectionConfig(mode, dist, buffer=buffer))

    for (w, h) in SIZES:
        xfs = frames(bounds, w, h)
        for n in (3, 4):
            for yi, y in enumerate((M.Y_UPWARD, M.Y_DOWNWARD)):
                for (mode, dist) in CONFIGS:
                    key = "%d_%d_%d_%d_%d_%d" % (w, h, n, yi, mode, dist)
                    st = torch.full((sub.n_glyphs, h, w), 77, dtype=torch.uint8, device="cuda")
                    out["tiles_"+key] = gb.generate(n, w, h, xfs, config=config(mode, dist), stencil=st, y_orientation=y).cpu().numpy()
                    out["stencil_"+key] = st.cpu().numpy()
    gb.close()
    for i, (w, h) in enumerate(SIZES):
        xfs = frames(bounds, w, h)
        g = single_glyph(i)
        for (mode, dist) in SINGLE_CONFIGS:
            st = np.full((h, w), 77, np.uint8)
            key = "%d_%d_%d_%d" % (w, h, mode, dist)
            out["single_"+key] = M.generate_msdf(np.zeros((h, w, 3), np.float32), sub.shape(g), M.SDFTransformation.from_xf(xfs[g]), config(mode, dist, buffer=st),
                                                 M.Y_DOWNWARD if i % 2 else M.Y_UPWARD)
            out["singlest_"+key] = st
    t = M.SDFTransformation.from_xf(np.array(W.XF, np.float64))
    for i, c in enumerate(shapeless_fields()):
        for p, fn in enumerate((M.msdf_fast_distance_error_correction, M.msdf_fast_edge_error_correction)):
            out["shapeless_%d_%d" % (i, p)] = fn(c["field"].copy(), t, W.RATIOS[i % len(W.RATIOS)])
    np.savez(out_path, **out)
    print("wrote %d arrays" % len(out))


if __name__ == "__main__":
    main(sys.argv[1])
