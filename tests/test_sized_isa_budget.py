"""Static budgets of k_distance_sized, the per-glyph-box twin of the dominant kernel (no GPU: hipcc cross-compiles one instantiation in a few seconds).

The twin runs k_distance's body with the glyph's own box loaded per workgroup (two wave-uniform dwords). It has to hold the budgets of
tests/test_kernel_isa_budget.py: the same occupancy, no more vector spills, and a hot edge loop without spill lane moves or scratch traffic -- and the
survivor records must still arrive by the hand-placed scalar batches (the loop this test finds is the one around the first s_load_dwordx16)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")


@pytest.mark.parametrize("inst,occupancy,max_vgpr_spill", [(("3", "true", "false", "4"), 4, 56),    # LDS class
                                                             (("3", "true", "true", "1"), 4, 96),     # global-scratch class (persistent grid)
                                                             (("3", "false", "false", "4"), 5, 0)])    # one-contour class
def test_edge_loop_of_k_distance_sized_has_no_spills(inst, occupancy, max_vgpr_spill):
    from isa_loop_depth import analyse
    a = analyse(*inst, kernel="k_distance_sized")
    res = a["resources"]
    print(res, a["edge_loop"])
    assert int(res["Occupancy"]) == occupancy, res
    assert int(res["VGPRs Spill"]) <= max_vgpr_spill, res
    e = a["edge_loop"]
    assert e is not None and e["lane moves"] <= 4 and e["scratch"] == 0 and e["f64 arithmetic"] > 300, e
    assert e["s_load"] == 5, e                             # R (two halves) + E0, then E1 + E2 of a curve: the records are still read with scalar loads
