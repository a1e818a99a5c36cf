"""The GPU side of tests/test_gpu_prep_plan.py, run by it as a child process under a time limit: every device call the test needs, results into one .npz.

    python tests/prepplan_gpu_child.py OUT.npz

want_<cfg>             GlyphBatch.from_raw(...) + generate(...) of the hand-built raw batch at 32x32 msdf: cfg "full" (ink-trap colouring, per-glyph seeds,
                       orient_contours, WINDING_GUESS, framed on the device) or "lean" (normalize off, colouring 0, no orientation, the caller's xf)
bounds_<cfg>           that batch's GlyphBatch.bounds()
stream_<cfg>_<chunk>   generate_stream of the same raw batch under the same configuration with that pipeline chunk (0: automatic, one chunk)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import orientcases as OC  # noqa: E402

SIZE = 32
CHUNKS = (0, 3, 1)


def raw_batch():
    return OC.hand_built_batch()


def seeds_of(n):
    return (np.arange(n, dtype=np.uint64)*np.uint64(2654435761)+np.uint64(11)) % np.uint64(1 << 40)


def lean_frames(raw):
    from msdfgen_amd.shape import autoframe
    return np.stack([autoframe(s.bounds() if s.n_edges else (0, 0, 1, 1), SIZE, SIZE, 4) for s in raw.shapes()])


def main(out_path):
    import msdfgen_amd as M
    from msdfgen_amd import lib as L
    M.init(0)
    assert M.device_info()["arch"].startswith("gfx950"), M.device_info()
    raw = raw_batch()
    seeds = seeds_of(raw.n_glyphs)
    configs = {
        "full": (M.PrepareConfig(True, 2, 3.0, 0, orient_contours=True, winding=M.WINDING_GUESS), seeds, None, M.FrameConfig(px_range=4)),
        "lean": (M.PrepareConfig(False, 0, 3.0, 0), None, lean_frames(raw), None),
    }
    out = {}
    lib = L.load()
    for name, (prep, sd, xfs, frame) in configs.items():
        gb = M.GlyphBatch.from_raw(raw, prep.normalize, prep.coloring, prep.angle_threshold, seeds=sd, seed=prep.seed, orient_contours=prep.orient_contours,
                                   winding=prep.winding)
        try:
            out["want_"+name] = gb.generate(M.MODE_MSDF, SIZE, SIZE, xfs, frame=frame).cpu().numpy()
            out["bounds_"+name] = gb.bounds()
        finally:
            gb.close()
        try:
            for chunk in CHUNKS:
                L.check(lib.msdfhip_set_pipeline_chunk(chunk))
                out["stream_%s_%d" % (name, chunk)] = M.generate_stream(raw, M.MODE_MSDF, SIZE, SIZE, xfs, prepare=prep, seeds=sd, frame=frame)
        finally:
            L.check(lib.msdfhip_set_pipeline_chunk(0))
    np.savez(out_path, **out)
    print("wrote %d arrays" % len(out))


if __name__ == "__main__":
    main(sys.argv[1])
