"""What a wavefront of k_ec_fast executes for the root loop of the diagonal artifact test (msdf_ec_fast.hpp: diagonalPairFast) on the bench workload, counted
on the CPU (profiles/ec_root_passes.md): an evenly spaced sample of tests/golden/dejavu8192.npz at 64x64 (the bench step's tiles, xf64), pre-correction
fields by the oracle, every 8x8 tile's item queue emulated in rounds of 64 by the host program of tests/ec_roots_host -- per-index root and extremum blocks
(before), in-range roots and extrema first (after), and the (item, root, test) units of a dense form.        python tools/ec_root_counts.py [--every 32]"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=32)
    args = ap.parse_args()
    import eclazycases as E
    import ecrootscases as R
    from oracle.pyoracle import Oracle
    cases = R.bench_cases(Oracle(), args.every)
    with tempfile.TemporaryDirectory() as tmp:
        status, r = R.run_host(R.build_host(tmp), cases, tmp)
    g = r["groups"][E.GROUP_BENCH]
    out = {"glyphs": len(cases), "mismatches": status, "comparisons": r["comparisons"], "items": g["items"], "rounds": g["rounds"]}
    rd = g["rounds"]
    out["per_round"] = {"rounds_per_tile": rd["rounds"]/rd["tiles"], "items_per_tile": rd["queued_items"]/rd["tiles"],
                        "linear_share_of_rounds": rd["rounds_with_linear"]/rd["rounds"], "lanes_reaching_loop": rd["lanes_reaching_loop"]/rd["rounds"],
                        "item_root_pairs": rd["item_root_pairs"]/rd["rounds"], "units": rd["units"]/rd["rounds"],
                        "before_body_executions": sum(rd["before_body"]), "before_extremum_executions": sum(rd["before_extremum_blocks"]),
                        "after_body_executions": sum(rd["after_passes"]),
                        "after_extremum_executions": rd["after_rounds_first_extremum"]+rd["after_rounds_second_extremum"]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
