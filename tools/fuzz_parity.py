"""Randomized parity sweep of the HIP path against the oracle, long form (run on the GPU box; `pytest -m gpu` runs bounded sweeps of the
same generator, tests/test_gpu_parity.py::test_fuzz_sweep_vs_oracle and tests/test_gpu_routes.py).  Prints one JSON line with the number of texel
values compared, the number differing bitwise and the worst |delta|; exit status 1 if any |delta| exceeds 1e-5 or a stencil / path byte differs.

    python tools/fuzz_parity.py [--shapes 1500] [--seed 1] [--single] [--framing mirror_x,aniso,...|all]
                                [--scale small|mixed|full] [--scanline] [--tuning NAME] [--stencil] [--paths]
                                [--geometry lattice_ties,coincident,...|all]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import fuzzlib
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=int, default=1500)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--single", action="store_true", help="every shape through its own generate*() call (the fused single-call launch) instead of batches")
    ap.add_argument("--framing", default=None, help="comma-separated framing families of tests/xformcases.py (or 'all') instead of autoframe")
    ap.add_argument("--scale", default="small", choices=("small", "mixed", "full"),
                    help="group sizes: small (the default sweep), mixed (40-80 glyphs of every class), full (>= 256 glyphs, > 8 192 tiles)")
    ap.add_argument("--scanline", action="store_true", help="every other group through the -scanline flow (sign pass), the fill rules in turn")
    ap.add_argument("--tuning", default=None, choices=sorted(fuzzlib.TUNINGS), help="a named MSDFHIP_* table of tests/fuzzlib.py (TUNINGS) for the run")
    ap.add_argument("--stencil", action="store_true", help="compare the error correction's stencils with the oracle's too")
    ap.add_argument("--paths", action="store_true", help="also run the groups through generate_stream and HostBatch.generate_host (bytes must match)")
    ap.add_argument("--geometry", default=None, help="comma-separated outline families of tests/geomcases.py (or 'all'), jittered on their lattice")
    args = ap.parse_args()
    geometry = None
    if args.geometry:
        import geomcases
        geometry = list(geomcases.FAMILIES) if args.geometry == "all" else args.geometry.split(",")
        bad = [f for f in geometry if f not in geomcases.FAMILIES]
        if bad:
            ap.error("unknown outline families %s; known: %s" % (bad, ", ".join(geomcases.FAMILIES)))
    framing = None
    if args.framing:
        import xformcases
        framing = list(xformcases.FAMILIES) if args.framing == "all" else args.framing.split(",")
        bad = [f for f in framing if f not in xformcases.FAMILIES]
        if bad:
            ap.error("unknown framing families %s; known: %s" % (bad, ", ".join(xformcases.FAMILIES)))
    r = fuzzlib.run(args.shapes, args.seed, single=args.single, framing=framing, scale=args.scale, scanline=args.scanline,
                    tuning=fuzzlib.TUNINGS[args.tuning] if args.tuning else None, stencil=args.stencil, paths=args.paths, geometry=geometry)
    r.pop("group_routes")
    print(json.dumps(r))
    sys.exit(1 if r["max_abs_delta"] > 1e-5 or (geometry and r["values_differing_bitwise"]) or r["stencil_values_differing"] or r["path_values_differing"] else 0)


if __name__ == "__main__":
    main()
