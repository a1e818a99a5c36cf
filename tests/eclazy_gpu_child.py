"""The GPU side of tests/test_gpu_ec_lazy.py, run by it as a child process under a time limit: every device call the test needs, results into one .npz.

    python tests/eclazy_gpu_child.py OUT.npz

pre_<w>_<h>_<n>_<y>                            pre-correction fields of the 40 fixture glyphs (error correction disabled), y: 0 upward, 1 downward rows
tiles_<w>_<h>_<n>_<y>_<mode>_<check>_<s>       GlyphBatch.generate under that configuration, s: 1 with a stencil buffer, 0 without
stencil_<w>_<h>_<n>_<y>_<mode>_<check>         the stencil buffer of the s = 1 call (filled with 77 before it)
single_<mode>_<check>_<g>_<y>, singlest_...    generate_msdf of glyph g alone at 23x17 (k_single_call), stencil through ErrorCorrectionConfig.buffer"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import eclazycases as E  # noqa: E402

SINGLE_SIZE = (23, 17)
SINGLE_CONFIGS = ((2, 1), (2, 0))                      # the lazy configuration and an eager one
CONFIGS = [(m, d) for m in E.MODES for d in E.DISTANCE_CHECKS]


def fixture():
    from msdfgen_amd.shape import ShapeBatch
    z = np.load(os.path.join(HERE, "golden", "latin.npz"))
    batch = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                       z["colors"].astype(np.int32), z["inverse_y"], [str(n) for n in z["names"]])
    picks = E.fixture_glyphs(batch.n_glyphs)
    return batch.select(picks), z["bounds"][picks]


def frames(bounds, w, h):
    return np.stack([E.frame(b, w, h) for b in bounds])


def single_glyphs(n):
    return range(0, n, 3)


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

    for (w, h) in E.GPU_SIZES:
        xfs = frames(bounds, w, h)
        for n in (3, 4):
            for yi, y in enumerate((M.Y_UPWARD, M.Y_DOWNWARD)):
                out["pre_%d_%d_%d_%d" % (w, h, n, yi)] = gb.generate(n, w, h, xfs, config=config(M.EC_DISABLED, 0), y_orientation=y).cpu().numpy()
                for (mode, dist) in CONFIGS:
                    key = "%d_%d_%d_%d_%d_%d" % (w, h, n, yi, mode, dist)
                    st = torch.full((sub.n_glyphs, h, w), 77, dtype=torch.uint8, device="cuda")
                    out["tiles_"+key+"_1"] = gb.generate(n, w, h, xfs, config=config(mode, dist), stencil=st, y_orientation=y).cpu().numpy()
                    out["stencil_"+key] = st.cpu().numpy()
                    out["tiles_"+key+"_0"] = gb.generate(n, w, h, xfs, config=config(mode, dist), y_orientation=y).cpu().numpy()
    gb.close()
    w, h = SINGLE_SIZE
    xfs = frames(bounds, w, h)
    for (mode, dist) in SINGLE_CONFIGS:
        for g in single_glyphs(sub.n_glyphs):
            for yi, y in enumerate((M.Y_UPWARD, M.Y_DOWNWARD)):
                st = np.full((h, w), 77, np.uint8)
                key = "%d_%d_%d_%d" % (mode, dist, g, yi)
                out["single_"+key] = M.generate_msdf(np.zeros((h, w, 3), np.float32), sub.shape(g), M.SDFTransformation.from_xf(xfs[g]), config(mode, dist, buffer=st), y)
                out["singlest_"+key] = st
    np.savez(out_path, **out)
    print("wrote %d arrays" % len(out))


if __name__ == "__main__":
    main(sys.argv[1])
