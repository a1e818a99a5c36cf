"""What the sized quality calls buy over the loops of uniform calls a caller had before them (profiles/sized_quality.md).

Workload: that of tools/sized_boxes_bench.py -- the bench's 8 192 distinct DejaVu glyphs at ONE common scale (--em-px texels per em), every glyph in its own
box; msdf fields from ONE generate_sized call, resident in HBM. Two measurements, each with two sides alternated --rounds times after --warmup untimed rounds
of each:

    estimate   sized: ONE msdfhip_batch_estimate_sdf_error_sized call over all glyphs
               loop:  one msdfhip_batch_estimate_sdf_error call per DISTINCT box size over that size's glyphs
    render     sized: ONE msdfhip_render_sdf_sized call, every box at --factor times its size, 1 <- 3 channels
               loop:  one msdfhip_render_sdf call per distinct box size

The sub-batches of the loops (uploaded and digested), their tiles (copies of the sized call's fields viewed (k, h, w, 3)), every descriptor array and every
output are made beforehand, outside the timing; both sides go through the C entry points with those, so neither pays for Python building descriptors. A round
is timed on the host clock between two device synchronizations: the sized calls do host work of their own (prefix, table upload, and they return when the
work has run), which belongs to what a caller waits for. Prints one JSON line: per measurement both sides' times (all rounds, median, spread = max - min),
the ratio of the medians and the number of values that differ bitwise between the sides (--no-check skips the comparison).

    python tools/sized_quality_bench.py [--em-px 32] [--range 4] [--spr 1] [--factor 2] [--rounds 7] [--warmup 2] [--glyphs 8192]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--em-px", type=float, default=32.)
    ap.add_argument("--range", type=float, default=4.)
    ap.add_argument("--spr", type=int, default=1)
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--glyphs", type=int, default=8192)
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()

    import torch
    import msdfgen_amd as M
    from msdfgen_amd import lib as L
    import bench
    from sized_boxes_bench import boxes
    M.init(0)
    lib = L.load()
    whole, _, _ = bench.load_dejavu()
    batch = whole.select(range(min(args.glyphs, whole.n_glyphs)))
    n = batch.n_glyphs
    gb = M.GlyphBatch(batch)
    sizes, xfs = boxes(gb.bounds(), args.em_px, args.range)
    sizes = np.ascontiguousarray(sizes, np.int32)
    offsets = M.GlyphBatch.packed_offsets(sizes, 3)
    tiles, _ = gb.generate_sized(3, sizes, xfs, config=M.MSDFGeneratorConfig())
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def error_descriptors(shapes, x):
        d = np.zeros(shapes.n_glyphs, L.GLYPH_DTYPE)
        d["xf"][:, :4] = x[:, :4]
        d["flip"] = shapes.inverse_y.astype(bool).astype(np.int32)
        return torch.from_numpy(d.view(np.uint8).reshape(shapes.n_glyphs, 64)).cuda()

    groups = {}
    for g, wh in enumerate(map(tuple, sizes.tolist())):
        groups.setdefault(wh, []).append(g)
    out_sizes = np.ascontiguousarray(sizes*args.factor, np.int32)
    out_offsets = M.GlyphBatch.packed_offsets(out_sizes, 1)
    subs = []
    for (w, h), idx in sorted(groups.items()):
        sub = M.GlyphBatch(batch.select(idx))
        t = torch.cat([tiles[int(offsets[g]):int(offsets[g+1])] for g in idx]).reshape(len(idx), h, w, 3).contiguous()
        subs.append((sub, w, h, idx, t, error_descriptors(sub.shapes, xfs[idx]), torch.empty(len(idx), dtype=torch.float64, device="cuda"),
                     torch.empty((len(idx), h*args.factor, w*args.factor, 1), dtype=torch.float32, device="cuda")))
    desc = error_descriptors(gb.shapes, xfs)
    errors = torch.empty(n, dtype=torch.float64, device="cuda")
    view = torch.empty(int(out_offsets[-1]), dtype=torch.float32, device="cuda")
    toff, ooff = np.ascontiguousarray(offsets[:-1]), np.ascontiguousarray(out_offsets[:-1])
    lo, hi = -.5*args.range, .5*args.range
    torch.cuda.synchronize()

    def estimate_sized():
        L.check(lib.msdfhip_batch_estimate_sdf_error_sized(gb._handle, 3, sizes.ctypes.data_as(i32), toff.ctypes.data_as(i64), desc.data_ptr(), tiles.data_ptr(), args.spr, 0,
                                                           errors.data_ptr(), None))

    def estimate_loop():
        for sub, w, h, _, t, d, e, _ in subs:
            L.check(lib.msdfhip_batch_estimate_sdf_error(sub._handle, 3, w, h, d.data_ptr(), t.data_ptr(), args.spr, 0, e.data_ptr(), None))

    def render_sized():
        L.check(lib.msdfhip_render_sdf_sized(tiles.data_ptr(), n, sizes.ctypes.data_as(i32), toff.ctypes.data_as(i64), 3, view.data_ptr(), out_sizes.ctypes.data_as(i32),
                                             ooff.ctypes.data_as(i64), 1, lo, hi, .5, None))

    def render_loop():
        for _, w, h, idx, t, _, _, o in subs:
            L.check(lib.msdfhip_render_sdf(t.data_ptr(), len(idx), w, h, 3, o.data_ptr(), w*args.factor, h*args.factor, 1, lo, hi, .5, None))

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter()-t0)*1e3

    def stats(v):
        return {"ms": [round(x, 4) for x in v], "median_ms": round(float(np.median(v)), 4), "spread_ms": round(max(v)-min(v), 4)}

    def measure(sized, loop):
        for _ in range(args.warmup):
            timed(sized), timed(loop)
        ms = {"sized": [], "loop": []}
        for _ in range(args.rounds):                                     # alternating: drift of the device hits both sides alike
            ms["sized"].append(timed(sized))
            ms["loop"].append(timed(loop))
        return {"sized": stats(ms["sized"]), "loop": stats(ms["loop"]), "loop_over_sized": round(float(np.median(ms["loop"])/np.median(ms["sized"])), 3)}

    res = {"workload": "dejavu8192", "glyphs": n, "em_px": args.em_px, "range_px": args.range, "mode": "msdf", "distinct_sizes": len(subs),
           "texels": int(offsets[-1]//3), "scanlines_per_row": args.spr, "render_factor": args.factor, "render_texels": int(out_offsets[-1])}
    res["estimate"] = measure(estimate_sized, estimate_loop)
    res["render"] = measure(render_sized, render_loop)
    if not args.no_check:
        e = errors.cpu().numpy().view(np.uint64)
        v = view.cpu().numpy().view(np.uint32)
        de = dv = 0
        for _, _, _, idx, _, _, se, so in subs:
            de += int((se.cpu().numpy().view(np.uint64) != e[idx]).sum())
            o = so.cpu().numpy().view(np.uint32)
            for k, g in enumerate(idx):
                dv += int((o[k].reshape(-1) != v[out_offsets[g]:out_offsets[g+1]]).sum())
        res["estimate"]["values_differing_bitwise"], res["render"]["values_differing_bitwise"] = de, dv
        res["estimate"]["mean_error"] = float(errors.mean().item())
    res["device"] = M.device_info()
    res["source_hash"] = __import__("msdfgen_amd.build", fromlist=["x"]).source_hash()
    for sub in subs:
        sub[0].close()
    gb.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
