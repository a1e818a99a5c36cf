"""Randomized parity sweep of the HIP path against the oracle, long form (run on the GPU box; `pytest -m gpu` runs a bounded sweep of the
same generator, tests/test_gpu_parity.py::test_fuzz_sweep_vs_oracle).  Prints one JSON line with the number of texel values compared,
the number differing bitwise and the worst |delta|; exit status 1 if any |delta| exceeds 1e-5.

    python tools/fuzz_parity.py [--shapes 1500] [--seed 1] [--single] [--framing mirror_x,aniso,...|all]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=1500)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--single", action="store_true", help="every shape through its own generate*() call (the fused single-call launch) instead of batches")
    ap.add_argument("--framing", default=None, help="comma-separated framing families of tests/xformcases.py (or 'all') instead of autoframe")
    args = ap.parse_args()
    import fuzzlib
    framing = None
    if args.framing:
        import xformcases
        framing = list(xformcases.FAMILIES) if args.framing == "all" else args.framing.split(",")
        bad = [f for f in framing if f not in xformcases.FAMILIES]
        if bad:
            ap.error("unknown framing families %s; known: %s" % (bad, ", ".join(xformcases.FAMILIES)))
    r = fuzzlib.run(args.shapes, args.seed, single=args.single, framing=framing)
    print(json.dumps(r))
    sys.exit(1 if r["max_abs_delta"] > 1e-5 else 0)


if __name__ == "__main__":
    main()
