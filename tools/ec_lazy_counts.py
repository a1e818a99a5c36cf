"""What the lazy protection order of k_ec_fast (msdf_ec_fast.hpp: ecLazyProtect) leaves to do on the bench workload, counted on the CPU before the kernel
was written (profiles/ec_lazy_protect.md): an evenly spaced sample of tests/golden/dejavu8192.npz at 64x64 (the bench step's tiles, xf64), pre-correction
fields by the oracle, walked by the host program of tests/ec_lazy_host. Per 8x8 tile: the texels whose protection the lazy order resolves, and the
protectEdges pairs the eager and the lazy order queue.        python tools/ec_lazy_counts.py [--every 64]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--every", type=int, default=64)
    args = ap.parse_args()
    import eclazycases as E
    from msdfgen_amd.shape import ShapeBatch
    from oracle.pyoracle import Oracle
    z = np.load(os.path.join(ROOT, "tests", "golden", "dejavu8192.npz"))
    batch = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                       z["colors"].astype(np.int32), np.zeros(8192, bool), [str(n) for n in z["names"]])
    orc = Oracle()
    cases = []
    for g in range(0, batch.n_glyphs, args.every):
        s = batch.shape(g)
        cases.append({"w": 64, "h": 64, "flip": int(bool(s.inverse_y)), "group": E.GROUP_BENCH, "shape": s, "xf": z["xf64"][g],
                      "field": orc.generate(s, 3, 64, 64, z["xf64"][g], ec_mode=0)})
    with tempfile.TemporaryDirectory() as tmp:
        status, r = E.run_host(E.build_host(tmp), cases, tmp)
    g = r["groups"][E.GROUP_BENCH]
    g["glyphs"], g["mismatches"] = len(cases), status
    print(json.dumps(g, indent=1))


if __name__ == "__main__":
    main()
