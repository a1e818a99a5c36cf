"""What msdfhip_batch_gather costs next to what a caller had before it (profiles/batch_gather.md).

Workload: the bench's 8 192 distinct DejaVu glyphs (tests/golden/dejavu8192.npz) resident in one GlyphBatch; selections of --sizes glyphs in shuffled order
(seeded; a selection of all glyphs is a permutation). Per selection two sides, alternated --rounds times after --warmup untimed rounds of each:

    gather  msdfhip_batch_gather on torch's current stream (the C call: no host mirror is built): `event_ms` between two stream events around the call
            (plan upload + copies + digest as the device sees them), `wall_ms` by the host clock from the call to the end of a stream synchronize (with the
            host plan, the allocations and the pinned table)
    create  msdfhip_batch_create from the host arrays of the same selection, which is synchronous: `wall_ms` by the host clock, flatten excluded (the arrays
            made beforehand) and `flatten_wall_ms` with ShapeBatch.select of the selection in front of it (what a caller without flat arrays pays)

Next to them, per selection: the digest alone (msdfhip_batch_digest on the gathered batch between two events, same rounds), the bytes the copy kernels
move (read + written: 66 B per edge, 4 B per contour offset, each twice, plus the table), and the rate they reach in what the gather's events leave after the
digest. The results of both sides are downloaded once and compared byte for byte.

Prints one JSON line.

    python tools/batch_gather_bench.py [--sizes 64,1024,8192] [--rounds 7] [--warmup 2] [--seed 1]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,8192")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import torch
    import msdfgen_amd as M
    from msdfgen_amd import lib as L
    import bench
    M.init(0)
    lib = L.load()
    whole, _, _ = bench.load_dejavu()
    gb = M.GlyphBatch(whole)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(args.seed)
    ip = L._ip

    def flat(sb):
        ne = max(sb.n_edges, 1)
        pts, types, colors = np.zeros((ne, 8), np.float64), np.ones(ne, np.uint8), np.zeros(ne, np.uint8)
        pts[:sb.n_edges], types[:sb.n_edges], colors[:sb.n_edges] = sb.points, sb.types, sb.colors
        return (np.ascontiguousarray(sb.glyph_contour_offsets, np.int32), np.ascontiguousarray(sb.contour_offsets, np.int32), pts, types, colors)

    def create(arrays, n):
        h = C.c_void_p()
        gco, co, pts, types, colors = arrays
        L.check(lib.msdfhip_batch_create(C.byref(h), n, L.ptr(gco, ip), L.ptr(co, ip), L.ptr(pts, L._dp), L.ptr(types, L._bp), L.ptr(colors, L._bp)))
        return h

    def gather(idx):
        h = C.c_void_p()
        src = (C.c_void_p*1)(gb._handle)
        L.check(lib.msdfhip_batch_gather(C.byref(h), src, 1, len(idx), None, L.ptr(idx, ip), stream.cuda_stream))
        return h

    def download(h, nc, ne):
        co, pts, types, colors = np.zeros(nc+1, np.int32), np.zeros((max(ne, 1), 8)), np.zeros(max(ne, 1), np.uint8), np.zeros(max(ne, 1), np.uint8)
        L.check(lib.msdfhip_batch_download(h, L.ptr(co, ip), L.ptr(pts, L._dp), L.ptr(types, L._bp), L.ptr(colors, L._bp)))
        w = np.zeros(max(nc, 1), np.int32)
        L.check(lib.msdfhip_batch_windings(h, L.ptr(w, ip)))
        return [a.tobytes() for a in (co, pts, types, colors, w)]

    def stats(v):
        return {"ms": [round(x, 4) for x in v], "median_ms": round(float(np.median(v)), 4), "spread_ms": round(max(v)-min(v), 4)}

    cases = []
    for n in (int(s) for s in args.sizes.split(",")):
        idx = np.ascontiguousarray(rng.permutation(whole.n_glyphs)[:n], np.int32)
        sub = whole.select(idx)
        arrays = flat(sub)
        ms = {"gather_event": [], "gather_wall": [], "digest_event": [], "create_wall": [], "create_flatten_wall": []}
        for r in range(args.warmup+args.rounds):                           # alternating: drift of the machine hits both sides alike
            torch.cuda.synchronize()
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            t0 = time.perf_counter()
            e0.record(stream)
            h = gather(idx)
            e1.record(stream)
            stream.synchronize()
            t1 = time.perf_counter()
            L.check(lib.msdfhip_batch_digest(h, stream.cuda_stream))
            e2.record(stream)
            stream.synchronize()
            t2 = time.perf_counter()
            hc = create(arrays, n)
            t3 = time.perf_counter()
            hf = create(flat(whole.select(idx)), n)
            t4 = time.perf_counter()
            if r == 0:
                same = download(h, sub.n_contours, sub.n_edges) == download(hc, sub.n_contours, sub.n_edges)
            for x in (h, hc, hf):
                lib.msdfhip_batch_destroy(x)
            if r >= args.warmup:
                ms["gather_event"].append(e0.elapsed_time(e1)), ms["gather_wall"].append(1e3*(t1-t0)), ms["digest_event"].append(e1.elapsed_time(e2))
                ms["create_wall"].append(1e3*(t3-t2)), ms["create_flatten_wall"].append(1e3*(t4-t3))
        moved = 2*(66*sub.n_edges+4*(sub.n_contours+1))+4*(n+1)+4*(5*n+1)
        copy_ms = float(np.median(ms["gather_event"]))-float(np.median(ms["digest_event"]))
        cases.append({"glyphs": n, "contours": sub.n_contours, "edges": sub.n_edges, "same_bytes_as_create": bool(same),
                      "gather_event": stats(ms["gather_event"]), "gather_wall": stats(ms["gather_wall"]), "digest_event": stats(ms["digest_event"]),
                      "create_wall": stats(ms["create_wall"]), "create_flatten_wall": stats(ms["create_flatten_wall"]),
                      "digest_share_of_gather_event": round(float(np.median(ms["digest_event"]))/float(np.median(ms["gather_event"])), 3),
                      "copy_bytes": moved, "copy_ms": round(copy_ms, 4), "copy_gb_per_s": round(moved/copy_ms/1e6, 2) if copy_ms > 0 else None,
                      "create_over_gather_wall": round(float(np.median(ms["create_wall"]))/float(np.median(ms["gather_wall"])), 2),
                      "create_flatten_over_gather_wall": round(float(np.median(ms["create_flatten_wall"]))/float(np.median(ms["gather_wall"])), 2)})
    res = {"workload": "dejavu8192", "resident_glyphs": gb.n_glyphs, "resident_edges": whole.n_edges, "rounds": args.rounds, "warmup": args.warmup, "cases": cases,
           "device": M.device_info(), "source_hash": __import__("msdfgen_amd.build", fromlist=["x"]).source_hash()}
    gb.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
