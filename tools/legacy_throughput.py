"""Device time of the legacy generators next to the modern simple route of the same build: GlyphBatch.generate_legacy(MODE_MSDF) against
GlyphBatch.generate(MODE_MSDF, overlap_support=False) on the 8 192-glyph DejaVu set at 64x64, both with the library-default error correction of their
route (legacy: without the distance check, as generateMSDF_legacy runs it). The two are timed alternately, each repetition between two stream events
after a warm-up; the medians, their ratio, and the two distance passes alone (error correction disabled) go out as one JSON line.

    python tools/legacy_throughput.py [--reps 15] [--out profiles/legacy_throughput.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import msdfgen_amd as M  # noqa: E402
from msdfgen_amd import build as B  # noqa: E402
from bench import load_dejavu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    M.init(0)
    batch, xf64, _ = load_dejavu()
    gb = M.GlyphBatch(batch)
    w = h = 64
    out = torch.empty((gb.n_glyphs, h, w, 3), dtype=torch.float32, device=gb.device)
    desc = gb.descriptors(xf64, w, h, 3)
    simple = M.MSDFGeneratorConfig(overlap_support=False)
    raw = M.MSDFGeneratorConfig(False, M.ErrorCorrectionConfig(M.EC_DISABLED))
    runs = {
        "legacy_msdf": lambda: gb.generate_legacy(M.MODE_MSDF, w, h, config=None, out=out, descriptors=desc),
        "modern_simple_msdf": lambda: gb.generate(M.MODE_MSDF, w, h, config=simple, out=out, descriptors=desc),
        "legacy_distance_only": lambda: gb.generate_legacy(M.MODE_MSDF, w, h, config=raw, out=out, descriptors=desc),
        "modern_simple_distance_only": lambda: gb.generate(M.MODE_MSDF, w, h, config=raw, out=out, descriptors=desc),
    }
    times = {k: [] for k in runs}
    for rep in range(args.warmup+args.reps):
        for name, fn in runs.items():                                # alternating: drift of the machine lands on all of them alike
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if rep >= args.warmup:
                times[name].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in times.items()}
    line = {"workload": "dejavu8192", "glyphs": gb.n_glyphs, "tile": [w, h], "mode": "msdf", "reps": args.reps, "source_hash": B.source_hash(),
            "median_ms": {k: round(v, 4) for k, v in med.items()}, "min_ms": {k: round(float(np.min(v)), 4) for k, v in times.items()},
            "max_ms": {k: round(float(np.max(v)), 4) for k, v in times.items()},
            "legacy_over_modern": round(med["legacy_msdf"]/med["modern_simple_msdf"], 3),
            "legacy_over_modern_distance_only": round(med["legacy_distance_only"]/med["modern_simple_distance_only"], 3)}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text+"\n")


if __name__ == "__main__":
    main()
