"""Raw outlines through the streamed generator: what preparing inside the chunk pipeline costs against streaming shapes that are prepared already.
One process, the 8 192 DejaVu glyphs of tests/golden/dejavu8192.npz, MSDF at 48x48 and 64x64, float tiles and the 8-bit atlas:
    (a) prepared   generate_stream of the fixture's prepared shapes (the path before raw input existed)
    (b) raw        generate_stream(prepare=PrepareConfig()) of the same outlines with every colour wiped to WHITE: normalize + edgeColoringSimple per
                   chunk on the device, inside the pipeline
    (c) cpu+a      the compiled reference's Shape::normalize + edgeColoringSimple on the host (oracle/_ref/libmsdfgen_ref.so through oracle.pyoracle.Ref,
                   a thread pool of --threads, as bench.py's CPU baseline), then (a)
    (d) raw+orient (b) with orient_contours=1, winding=guess: k_prep_orient before normalize, k_prep_winding after it
    (e) cpu-orient+a  (c) with the reference's orientContours before normalize and the -guesswinding step after it (tests/orientcases.py), then (a)
Every (size, output, variant) is warmed up first; the timed calls are interleaved round-robin, --reps of each; median / min / max per cell.
(b)'s bytes are checked against (a)'s once per cell (the fixture's shapes are what the reference's preparation gives the wiped set).
--perturb: the raw variants stream the outlines with every contour of every 3rd glyph and one contour of every 5th reversed (orientcases.perturbed).
    python tools/stream_raw_bench.py [--reps 9] [--out profiles/NAME_stream_raw.jsonl]
    python tools/stream_raw_bench.py --only raw --reps 3 --sizes 48 --outputs uint8      (one variant alone: for rocprofv3 runs)"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import msdfgen_amd as M  # noqa: E402
from msdfgen_amd.shape import FlatShape, ShapeBatch  # noqa: E402


def load_sets():
    z = np.load(os.path.join(ROOT, "tests", "golden", "dejavu8192.npz"))
    prepared = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                          z["colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    raw = ShapeBatch(prepared.glyph_contour_offsets, prepared.contour_offsets, prepared.points, prepared.types, np.full(prepared.n_edges, 7, np.int32),
                     prepared.inverse_y, prepared.names)
    return prepared, raw, {48: z["xf48"], 64: z["xf64"]}


def cpu_prepare(ref, raw, pool):
    """The reference's normalize + edgeColoringSimple(3.0, seed 0) of every glyph on the pool, concatenated into one CSR batch."""
    fas = list(pool.map(lambda g: ref.shape_prepare(raw.shape(g), True, 1, 3.0, 0), range(raw.n_glyphs), chunksize=64))
    return ShapeBatch.from_shapes([FlatShape(f.contour_offsets, f.points, f.types, f.colors) for f in fas])


def cpu_prepare_oriented(ref, raw, pool):
    """(e)'s host preparation: orientContours, normalize, the winding guess, edgeColoringSimple(3.0, seed 0) -- the reference's, glyph by glyph."""
    import orientcases as OC
    fas = list(pool.map(lambda g: OC.ref_prepare(ref, raw.shape(g), True, 2, True, 1, 3.0, 0), range(raw.n_glyphs), chunksize=64))
    return ShapeBatch.from_shapes(fas)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="48,64")
    ap.add_argument("--outputs", default="uint8,float")
    ap.add_argument("--only", choices=("prepared", "raw", "cpu+a", "raw+orient", "cpu-orient+a"), default=None)
    ap.add_argument("--perturb", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="jsonl file (one line per cell)")
    args = ap.parse_args()
    M.init(0)
    prepared, raw, xfs = load_sets()
    n = raw.n_glyphs
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if args.perturb:
        import orientcases as OC
        raw = OC.perturbed(raw)
    prep = M.PrepareConfig(True, 1, 3.0, 0)
    prep_orient = M.PrepareConfig(True, 1, 3.0, 0, orient_contours=True, winding=M.WINDING_GUESS)
    variants = [args.only] if args.only else ["prepared", "raw", "cpu+a", "raw+orient", "cpu-orient+a"]
    ref, pool, cpu_impl = None, None, None
    if "cpu+a" in variants or "cpu-orient+a" in variants:
        from oracle.pyoracle import Ref, Oracle
        ref = Ref() if Ref.available() else Oracle()
        cpu_impl = "compiled reference (oracle/_ref/libmsdfgen_ref.so)" if isinstance(ref, Ref) else "oracle C port (reference not built)"
        pool = ThreadPoolExecutor(args.threads)
    env = {"GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES", "unset (HIP default 4)")}
    lines = []
    for size in [int(s) for s in args.sizes.split(",")]:
        xf = xfs[size]
        for output in args.outputs.split(","):
            tile = size*size*3
            offs = np.arange(n, dtype=np.int64)*tile
            buf = M.host_alloc((n, size, size, 3), np.uint8 if output == "uint8" else np.float32)   # pinned, as an atlas tool would use

            def stream(shapes, **kw):
                if output == "uint8":
                    M.generate_stream(shapes, M.MODE_MSDF, size, size, xf, atlas=buf, out_offsets=offs, row_stride=size*3, **kw)
                else:
                    M.generate_stream(shapes, M.MODE_MSDF, size, size, xf, out=buf, **kw)

            def run(v):
                if v == "prepared":
                    stream(prepared)
                elif v == "raw":
                    stream(raw, prepare=prep)
                elif v == "raw+orient":
                    stream(raw, prepare=prep_orient)
                elif v == "cpu+a":
                    stream(cpu_prepare(ref, raw, pool))
                else:
                    stream(cpu_prepare_oriented(ref, raw, pool))

            for v in variants:                                       # warm-up: pools, pipes, staging grown, kernels loaded
                run(v)
            if args.only is None:
                stream(prepared)
                want = buf.copy()
                stream(raw, prepare=prep)
                same = bool((buf.view(np.uint8) == want.view(np.uint8)).all())
            else:
                same = None
            times = {v: [] for v in variants}
            for _ in range(args.reps):
                for v in variants:
                    t0 = time.perf_counter()
                    run(v)
                    times[v].append((time.perf_counter()-t0)*1e3)
            M.host_free(buf)
            for v in variants:
                t = np.array(times[v])
                line = {"tool": "stream_raw_bench", "glyphs": n, "size": size, "output": output, "variant": v, "reps": args.reps,
                        "median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t.min()), 3), "max_ms": round(float(t.max()), 3),
                        "glyphs_per_s": round(n/float(np.median(t))*1e3), "raw_equals_prepared": same, "perturbed": args.perturb, **env}
                if v in ("cpu+a", "cpu-orient+a"):
                    line["cpu_prepare"] = "%s, %d threads" % (cpu_impl, args.threads)
                lines.append(line)
                print(json.dumps(line), flush=True)
            if args.only is None:
                a, b = np.median(times["prepared"]), np.median(times["raw"])
                print("# %dx%d %s: raw / prepared = %.3f, raw+orient - raw = %.3f ms" % (size, size, output, b/a, np.median(times["raw+orient"])-b), flush=True)
    if pool:
        pool.shutdown()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line)+"\n")


if __name__ == "__main__":
    main()
