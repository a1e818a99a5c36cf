"""What GlyphBatch.boxes() costs next to the host route a caller had before it (profiles/boxes.md).

Workload: the bench's 8 192 distinct DejaVu glyphs (tests/golden/dejavu8192.npz) resident in one GlyphBatch, boxes at --em-px texels per em with a pixel
range of --range. Two sides, alternated --rounds times after --warmup untimed rounds of each, each timed with the host clock around the whole call (both
end in a device-to-host copy, so both are synchronous):

    device  GlyphBatch.boxes(BoxConfig(em_px, px_range, miter_limit)): one k_box launch, one copy back of sizes, transformations and bounds
    host    GlyphBatch.bounds() + the NumPy rule of tools/sized_boxes_bench.py: boxes() (plain bounds only: the host route has no miters at all)

Prints one JSON line: both sides' times (all rounds, median, spread = max - min), how many boxes the miter limit enlarges over limit 0 (sizes compared), by
how many texels in all, and how many glyphs have no box.

    python tools/boxes_bench.py [--em-px 32] [--range 4] [--miter-limit 4] [--rounds 9] [--warmup 3] [--glyphs 8192]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--em-px", type=float, default=32.)
    ap.add_argument("--range", type=float, default=4.)
    ap.add_argument("--miter-limit", type=float, default=4.)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--glyphs", type=int, default=8192)
    args = ap.parse_args()

    import torch
    import msdfgen_amd as M
    import bench
    from sized_boxes_bench import boxes as host_boxes
    M.init(0)
    whole, _, _ = bench.load_dejavu()
    batch = whole.select(range(min(args.glyphs, whole.n_glyphs)))
    gb = M.GlyphBatch(batch)
    torch.cuda.synchronize()
    cfg = M.BoxConfig(args.em_px, px_range=args.range, miter_limit=args.miter_limit)

    def device():
        return gb.boxes(cfg)

    def host():
        return host_boxes(gb.bounds(), args.em_px, args.range)

    def timed(f):
        t0 = time.perf_counter()
        f()
        return 1e3*(time.perf_counter()-t0)

    for _ in range(args.warmup):
        timed(device), timed(host)
    ms = {"device": [], "host": []}
    for _ in range(args.rounds):                                         # alternating: drift of the machine hits both sides alike
        ms["device"].append(timed(device))
        ms["host"].append(timed(host))
    with_miters = gb.boxes(cfg)[0].astype(np.int64)
    without = gb.boxes(M.BoxConfig(args.em_px, px_range=args.range, miter_limit=0.))[0].astype(np.int64)
    larger = (with_miters != without).any(1)

    def stats(v):
        return {"ms": [round(x, 4) for x in v], "median_ms": round(float(np.median(v)), 4), "spread_ms": round(max(v)-min(v), 4)}
    res = {"workload": "dejavu8192", "glyphs": gb.n_glyphs, "edges": batch.n_edges, "em_px": args.em_px, "range_px": args.range, "miter_limit": args.miter_limit,
           "device_boxes": stats(ms["device"]), "host_bounds_numpy": stats(ms["host"]),
           "host_over_device": round(float(np.median(ms["host"])/np.median(ms["device"])), 3), "boxes_enlarged_by_miters": int(larger.sum()),
           "texels_without_miters": int((without[:, 0]*without[:, 1]).sum()), "texels_with_miters": int((with_miters[:, 0]*with_miters[:, 1]).sum()),
           "glyphs_without_box": int((with_miters == 0).all(1).sum()), "device": M.device_info(),
           "source_hash": __import__("msdfgen_amd.build", fromlist=["x"]).source_hash()}
    gb.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
