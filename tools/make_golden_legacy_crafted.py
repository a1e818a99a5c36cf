#!/usr/bin/env python3
"""Records tests/golden/legacy_crafted.npz: the crafted fields of tests/legacycases.py (crafted_fields: infinities, NaN, -0, equalized texels, neighbour
differences at and one ulp around the thresholds) and what the compiled reference's msdfErrorCorrection_legacy makes of them -- data only, for the tests
that have no reference at hand (tests/test_gpu_legacy_cases.py). Needs oracle/_ref/libmsdfgen_ref.so (make -C oracle).

    python tools/make_golden_legacy_crafted.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import legacycases as LC  # noqa: E402
from oracle.pyoracle import Ref  # noqa: E402


def main():
    rl = LC.RefLegacy(Ref())
    fields = LC.crafted_fields()
    outs = [rl.correction(e.field, e.tx, e.ty) for e in fields]
    changed = sum(LC.differing(o, e.field) for o, e in zip(outs, fields))
    assert changed > 0, "the reference corrected nothing"
    offs = np.cumsum([0]+[e.field.size for e in fields])[:-1]
    path = os.path.join(ROOT, "tests", "golden", "legacy_crafted.npz")
    np.savez_compressed(path, ec_n=np.array([e.n for e in fields], np.int32), ec_w=np.array([e.w for e in fields], np.int32),
                        ec_h=np.array([e.h for e in fields], np.int32), ec_tx=np.array([e.tx for e in fields]), ec_ty=np.array([e.ty for e in fields]),
                        ec_off=offs.astype(np.int64), ec_in=np.concatenate([e.field.ravel() for e in fields]),
                        ec_out=np.concatenate([o.ravel() for o in outs]))
    print("%s: %d fields, %d values, %d changed by the reference, %d bytes" % (path, len(fields), int(sum(e.field.size for e in fields)), changed,
                                                                               os.path.getsize(path)))


if __name__ == "__main__":
    main()
