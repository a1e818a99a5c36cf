"""The GPU side of tests/test_gpu_ec_hw_median.py, run by it as a child process under a time limit: every device call the test needs, results into one .npz.

    python tests/echwmed_gpu_child.py OUT.npz

shapeless_<name>_<p>     field <name> of tests/echwmedcases.py: gpu_cases through msdf_fast_distance_error_correction (p = 0) / msdf_fast_edge_error_correction (p = 1)
pair_<round>_<k>         four fields (two with a -inf texel, two finite) corrected by four host threads at once with ONE leader slot: the first call runs
                         alone, the calls that queue up behind it are merged into one batch of two or three glyphs (msdfgen_hip.h: micro-batching;
                         which calls meet is up to the scheduler); pair_largest = the largest batch that formed
tiles, stencil           GlyphBatch.generate of two fixture glyphs (the smallest two-contour shape first), msdf 16x16, default configuration, with a stencil"""
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import echwmedcases as H  # noqa: E402
import ecwordscases as W  # noqa: E402

PAIR_ROUNDS = 4
PAIR_FIELDS = ("neginf_inner_16x16_0", "wave_16x16_1", "neginf_edge_16x16_2", "wave_16x16_0")
GLYPH_SIZE = 16


def fixture():
    """Two Basic-Latin fixture glyphs: the two-contour shape with the fewest edges, and the one after it in that order."""
    from msdfgen_amd.shape import ShapeBatch
    z = np.load(os.path.join(HERE, "golden", "latin.npz"))
    batch = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                       z["colors"].astype(np.int32), z["inverse_y"], [str(n) for n in z["names"]])
    gco, co = z["glyph_contour_offsets"].astype(np.int64), z["contour_offsets"].astype(np.int64)
    two = [g for g in range(batch.n_glyphs) if gco[g+1]-gco[g] == 2]
    two.sort(key=lambda g: (int(co[gco[g+1]]-co[gco[g]]), g))
    picks = np.array(two[:2])
    return batch.select(picks), z["bounds"][picks]


def frames(bounds):
    from msdfgen_amd.shape import autoframe
    return np.stack([autoframe(b, GLYPH_SIZE, GLYPH_SIZE, 2.) for b in bounds])


def main(out_path):
    import torch
    import msdfgen_amd as M
    M.init(0)
    assert M.device_info()["arch"].startswith("gfx950"), M.device_info()
    out = {}
    t = M.SDFTransformation.from_xf(np.array(W.XF, np.float64))
    cases = H.gpu_cases()
    for name, field in cases.items():
        for p, fn in enumerate((M.msdf_fast_distance_error_correction, M.msdf_fast_edge_error_correction)):
            out["shapeless_%s_%d" % (name, p)] = fn(np.ascontiguousarray(field).copy(), t, W.RATIOS[0])

    sub, bounds = fixture()
    gb = M.GlyphBatch(sub)
    st = torch.full((sub.n_glyphs, GLYPH_SIZE, GLYPH_SIZE), 77, dtype=torch.uint8, device="cuda")
    out["tiles"] = gb.generate(3, GLYPH_SIZE, GLYPH_SIZE, frames(bounds), stencil=st).cpu().numpy()
    out["stencil"] = st.cpu().numpy()
    gb.close()
    M.set_microbatch(256, 1)                                     # (last in this process: the setting is not restored)
    M.microbatch_stats(reset=True)
    for r in range(PAIR_ROUNDS):
        fields = [np.ascontiguousarray(cases[n]).copy() for n in PAIR_FIELDS]
        gate = threading.Barrier(len(fields))

        def work(f):
            gate.wait()
            M.msdf_fast_distance_error_correction(f, t, W.RATIOS[0])

        threads = [threading.Thread(target=work, args=(f,)) for f in fields]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        for k, f in enumerate(fields):
            out["pair_%d_%d" % (r, k)] = f
    out["pair_largest"] = np.array(M.microbatch_stats()["largest"])

    np.savez(out_path, **out)
    print("wrote %d arrays, largest concurrent batch %d" % (len(out), int(out["pair_largest"])))


if __name__ == "__main__":
    main(sys.argv[1])
