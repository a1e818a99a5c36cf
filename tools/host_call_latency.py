"""Latency / throughput of the literal drop-in call (single shape, host pointers in and out, PCIe both ways) from one host thread
and from a pool of C++ host threads -- the way msdf-atlas-gen's workers call generateMSDF -- with the library's micro-batcher on
and off.  Reported in DESIGN.md (it is never bench.py's value).

    python tools/host_call_latency.py [--threads 1,4,16,64] [--calls 400] [--boxes]

--boxes: every call takes its glyph's OWN bitmap size -- GlyphBatch.boxes at 32 texels per em on the bench's DejaVu set (tests/golden/dejavu8192.npz),
or the BOXES cycle of tests/test_gpu_sized.py over the Basic-Latin glyphs where that file is absent. The mode uses only entry points and binding
functions that predate the grouping of different sizes, so the same tool measures a checkout of an earlier commit (profiles/microbatch_sizes.md).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "tools", "hostbench")
SO = os.path.join(HERE, "libhostbench.so")


def build():
    from msdfgen_amd import build as B
    B.build_lib()
    src = os.path.join(HERE, "hostbench.cpp")
    if not os.path.exists(SO) or os.path.getmtime(src) > os.path.getmtime(SO):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", os.path.join(ROOT, "include"), src, "-o", SO,
                        "-L", B.LIBDIR, "-lmsdfgen_hip", "-Wl,-rpath," + B.LIBDIR], check=True)
    return SO


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", default="1,4,16,64")
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--leaders", default="4,0", help="micro-batcher leader slots per run; 0 = micro-batching off")
    ap.add_argument("--boxes", action="store_true", help="every call at its glyph's own box size instead of 64 x 64")
    ap.add_argument("--em-px", type=float, default=32.)
    ap.add_argument("--glyphs", type=int, default=8192, help="--boxes: the first N glyphs of the set")
    args = ap.parse_args()
    import msdfgen_amd as M
    from msdfgen_amd.shape import distance_mapping
    M.init(0)
    hb = C.CDLL(build())
    hb.hostbench_run.restype = C.c_double
    z = np.load(os.path.join(ROOT, "tests", "golden", "latin.npz"))
    gco = np.ascontiguousarray(z["glyph_contour_offsets"], np.int32)
    co = np.ascontiguousarray(z["contour_offsets"], np.int32)
    pts = np.ascontiguousarray(z["points"], np.float64)
    types = np.ascontiguousarray(z["types"], np.uint8)
    colors = np.ascontiguousarray(z["colors"], np.uint8)
    xfs = np.array([[x[0], x[1], x[2], x[3], *distance_mapping(x[4], x[5])] for x in z["xf64"]], np.float64)
    G = len(gco)-1
    sizes = None
    if args.boxes:
        if os.path.exists(os.path.join(ROOT, "tests", "golden", "dejavu8192.npz")):
            import bench
            whole, _, _ = bench.load_dejavu()
            batch = whole.select(range(min(args.glyphs, whole.n_glyphs)))
            gb = M.GlyphBatch(batch)
            sizes, xfs, _ = gb.boxes(M.BoxConfig(args.em_px, px_range=4., miter_limit=4.))
            gb.close()
            gco, co = np.ascontiguousarray(batch.glyph_contour_offsets, np.int32), np.ascontiguousarray(batch.contour_offsets, np.int32)
            pts, types, colors = np.ascontiguousarray(batch.points, np.float64), np.ascontiguousarray(batch.types, np.uint8), np.ascontiguousarray(batch.colors, np.uint8)
        else:
            from msdfgen_amd.shape import autoframe
            cycle = ((1, 1), (7, 9), (8, 8), (9, 8), (8, 9), (24, 1), (1, 17), (23, 17), (16, 16), (17, 10), (24, 17))
            sizes = np.array([cycle[g % len(cycle)] for g in range(G)], np.int32)
            framed = [autoframe(b, int(w), int(h), min(2., .5*min(int(w), int(h)))) for b, (w, h) in zip(z["bounds"], sizes)]
            xfs = np.array([[x[0], x[1], x[2], x[3], *distance_mapping(x[4], x[5])] for x in framed], np.float64)
        sizes, xfs = np.ascontiguousarray(sizes, np.int32), np.ascontiguousarray(xfs, np.float64)
        G = len(gco)-1
        hb.hostbench_run_boxes.restype = C.c_double

    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t))

    def run(nt, calls):
        bad = C.c_int()
        if sizes is not None:
            secs = hb.hostbench_run_boxes(nt, calls, G, p(gco, C.c_int32), p(co, C.c_int32), p(pts, C.c_double), p(types, C.c_uint8), p(colors, C.c_uint8),
                                          p(xfs, C.c_double), 3, p(sizes, C.c_int32), C.byref(bad))
            assert bad.value == 0, "%d calls failed" % bad.value
            return secs
        tile = np.zeros((64, 64, 3), np.float32)
        secs = hb.hostbench_run(nt, calls, G, p(gco, C.c_int32), p(co, C.c_int32), p(pts, C.c_double), p(types, C.c_uint8), p(colors, C.c_uint8),
                                p(xfs, C.c_double), 3, 64, 64, C.byref(bad), p(tile, C.c_float))
        assert bad.value == 0, "%d calls failed" % bad.value
        return secs
    for micro in [int(x) for x in args.leaders.split(",")]:
        M.set_microbatch(256 if micro else 1, max(micro, 1))
        run(4, 20)                                                       # warm the arenas
        for nt in [int(t) for t in args.threads.split(",")]:
            M.microbatch_stats(reset=True)
            secs = run(nt, args.calls)
            st = M.microbatch_stats()
            ph = (C.c_double*8)()
            M.load().msdfhip_debug_single_call_phases(ph, 1)
            mixed = {k: st[k] for k in ("mixed_batches", "mixed_calls", "padded_texels", "box_texels") if k in st}   # (absent from builds that group equal sizes only)
            print(json.dumps({"boxes": bool(args.boxes), **mixed, "leaders": micro, "host_threads": nt, "calls": nt*args.calls, "us_per_call_per_thread": round(1e6*secs/args.calls, 1),
                              "glyphs_per_s": round(nt*args.calls/secs), "device_batches": st["batches"], "largest_group": st["largest"],
                              "us_per_batch": {k: round(1e3*st[k+"_ms"]/max(st["batches"], 1), 1) for k in ("stage", "device", "scatter")},
                              "fused_single_calls": int(ph[0]), "fused_shader_mhz": round((ph[0]-int(ph[0]))*1e6), "fused_phase_us": dict(zip(("digest", "distance_wg0", "wait_all_tiles", "sweep_wg0", "candidates_visible", "checks_wg0", "first_to_last"),
                                                                                        [round(v, 2) for v in list(ph)[1:]]))}), flush=True)


if __name__ == "__main__":
    main()
