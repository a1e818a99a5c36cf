"""The GPU side of tests/test_gpu_ec_emit_mask.py, run by it as a child process under a time limit: every device call the test needs, results into one .npz.

    python tests/ecemitmask_gpu_child.py OUT.npz

shapeless_<name>_<p>     field <name> of tests/ecemitmaskcases.py: gpu_cases through msdf_fast_distance_error_correction (p = 0) / msdf_fast_edge_error_correction (p = 1)
tiles_<c>, stencil_<c>   GlyphBatch.generate of two fixture glyphs (tests/echwmed_gpu_child.py: fixture), msdf 16x16, with a stencil: c = 0 the default
                         configuration (the lazy order, with distance-check candidates), c = 1 EDGE_PRIORITY without the distance check (the eager order: protect
                         queue and find queue in one phase A)
counts_0                 msdfhip_batch_candidate_counts after the default run: overflow flag, then the distance-check candidates of each glyph"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ecemitmaskcases as E  # noqa: E402
import echwmed_gpu_child as G  # noqa: E402
import ecwordscases as W  # noqa: E402


def glyph_configs(M):
    return (M.MSDFGeneratorConfig(True, M.ErrorCorrectionConfig()),
            M.MSDFGeneratorConfig(True, M.ErrorCorrectionConfig(M.EC_EDGE_PRIORITY, M.DO_NOT_CHECK_DISTANCE)))


def main(out_path):
    import torch
    import msdfgen_amd as M
    M.init(0)
    assert M.device_info()["arch"].startswith("gfx950"), M.device_info()
    out = {}
    t = M.SDFTransformation.from_xf(np.array(W.XF, np.float64))
    for name, field in E.gpu_cases().items():
        for p, fn in enumerate((M.msdf_fast_distance_error_correction, M.msdf_fast_edge_error_correction)):
            out["shapeless_%s_%d" % (name, p)] = fn(np.ascontiguousarray(field).copy(), t, W.RATIOS[0])

    sub, bounds = G.fixture()
    gb = M.GlyphBatch(sub)
    s = G.GLYPH_SIZE
    for c, config in enumerate(glyph_configs(M)):
        st = torch.full((sub.n_glyphs, s, s), 77, dtype=torch.uint8, device="cuda")
        out["tiles_%d" % c] = gb.generate(3, s, s, G.frames(bounds), config=config, stencil=st).cpu().numpy()
        out["stencil_%d" % c] = st.cpu().numpy()
        if c == 0:
            overflow, counts = gb.candidate_counts()
            out["counts_0"] = np.concatenate([[int(overflow)], np.asarray(counts, np.int64)])
    gb.close()
    np.savez(out_path, **out)
    print("wrote %d arrays" % len(out))


if __name__ == "__main__":
    main(sys.argv[1])
