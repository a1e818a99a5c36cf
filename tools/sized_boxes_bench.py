"""What one generate_sized call buys over the loop of uniform calls a caller had before it (profiles/sized_boxes.md).

Workload: the bench's 8 192 distinct DejaVu glyphs (tests/golden/dejavu8192.npz) at ONE common scale (--em-px texels per em), every glyph in its own box =
its bounds (GlyphBatch.bounds(), the device's Shape::getBounds) at that scale plus --range texels, as an atlas generator sizes them; msdf, library-default
config, outputs resident in HBM. Two sides, alternated --rounds times after --warmup untimed rounds of each:

    sized   ONE GlyphBatch.generate_sized call over all glyphs
    loop    one GlyphBatch.generate call per DISTINCT box size over that size's glyphs (sub-batches uploaded and digested beforehand, outside the timing)

Every round is timed with events on the stream around the whole side and ends with a synchronize. Prints one JSON line: both sides' times (all rounds,
median, spread = max - min), the number of distinct sizes, and sum(w_g*h_g) / (n*W*H) -- the share of the padded grid that is real work. The two sides' floats
are compared bit for bit once (--no-check skips it).

    python tools/sized_boxes_bench.py [--em-px 32] [--range 4] [--rounds 7] [--warmup 2] [--glyphs 8192]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def boxes(bounds, em_px, px_range):
    """(sizes (G, 2) int32, xfs (G, 6)): every glyph's bounds at em_px texels per unit, centred in a box of ceil(extent + range) texels a side."""
    l, b, r, t = (bounds[:, k] for k in range(4))
    empty = (l >= r) | (b >= t)
    l, b, r, t = (np.where(empty, v, a) for v, a in ((0., l), (0., b), (0., r), (0., t)))
    w = np.maximum(np.ceil((r-l)*em_px+px_range), 1).astype(np.int32)
    h = np.maximum(np.ceil((t-b)*em_px+px_range), 1).astype(np.int32)
    xfs = np.zeros((len(l), 6))
    xfs[:, 0] = xfs[:, 1] = em_px
    xfs[:, 2] = .5*(w/em_px-(r-l))-l                                    # texel x = em_px*(shape x + translate)
    xfs[:, 3] = .5*(h/em_px-(t-b))-b
    xfs[:, 4], xfs[:, 5] = -.5*px_range/em_px, .5*px_range/em_px
    return np.stack([w, h], 1), xfs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--em-px", type=float, default=32.)
    ap.add_argument("--range", type=float, default=4.)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--glyphs", type=int, default=8192)
    ap.add_argument("--no-check", action="store_true")
    args = ap.parse_args()

    import torch
    import msdfgen_amd as M
    import bench
    M.init(0)
    whole, _, _ = bench.load_dejavu()
    batch = whole.select(range(min(args.glyphs, whole.n_glyphs)))
    n = batch.n_glyphs
    gb = M.GlyphBatch(batch)
    sizes, xfs = boxes(gb.bounds(), args.em_px, args.range)
    W, H = int(sizes[:, 0].max()), int(sizes[:, 1].max())
    share = float((sizes[:, 0].astype(np.int64)*sizes[:, 1]).sum())/(n*W*H)
    cfg = M.MSDFGeneratorConfig()
    offsets = M.GlyphBatch.packed_offsets(sizes, 3)
    out = torch.empty(int(offsets[-1]), dtype=torch.float32, device="cuda")
    desc = gb.descriptors_sized(xfs, sizes, 3)

    groups = {}
    for g, wh in enumerate(map(tuple, sizes.tolist())):
        groups.setdefault(wh, []).append(g)
    subs = []
    for (w, h), idx in sorted(groups.items()):
        sub = M.GlyphBatch(batch.select(idx))
        subs.append((sub, w, h, sub.descriptors(xfs[idx], w, h, 3), torch.empty((len(idx), h, w, 3), dtype=torch.float32, device="cuda"), idx))
    torch.cuda.synchronize()

    def sized():
        gb.generate_sized(3, sizes, config=cfg, out=out, descriptors=desc)

    def loop():
        for sub, w, h, d, o, _ in subs:
            sub.generate(3, w, h, config=cfg, out=o, descriptors=d)

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _ in range(args.warmup):
        timed(sized), timed(loop)
    ms = {"sized": [], "loop": []}
    for _ in range(args.rounds):                                         # alternating: drift of the device hits both sides alike
        ms["sized"].append(timed(sized))
        ms["loop"].append(timed(loop))
    differing = None
    if not args.no_check:
        flat = out.cpu().numpy().view(np.uint32)
        differing = 0
        for sub, w, h, d, o, idx in subs:
            tiles = o.cpu().numpy().view(np.uint32)
            for k, g in enumerate(idx):
                differing += int((tiles[k].reshape(-1) != flat[offsets[g]:offsets[g+1]]).sum())

    def stats(v):
        return {"ms": [round(x, 4) for x in v], "median_ms": round(float(np.median(v)), 4), "spread_ms": round(max(v)-min(v), 4)}
    res = {"workload": "dejavu8192", "glyphs": n, "em_px": args.em_px, "range_px": args.range, "mode": "msdf", "slot": [W, H], "distinct_sizes": len(subs),
           "padded_grid_share_of_real_work": round(share, 4), "texels": int(offsets[-1]//3), "sized": stats(ms["sized"]), "loop": stats(ms["loop"]),
           "loop_over_sized": round(float(np.median(ms["loop"])/np.median(ms["sized"])), 3), "values_differing_bitwise": differing,
           "device": M.device_info(), "source_hash": __import__("msdfgen_amd.build", fromlist=["x"]).source_hash()}
    for sub in subs:
        sub[0].close()
    gb.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
