"""Static budget of both instantiations of k_ec_fast (no GPU: hipcc cross-compiles one instantiation in a few seconds).

The lazy protection order keeps more scalar values alive across phase C than the eager one; the late round therefore reads the glyph's parameters again
behind a compiler barrier (msdf_kernels.hpp: ecFastBody), and what does not fit is parked in lanes of a vector register. That is register allocation
by hand for one compiler, so the outcome is pinned here: at most 72 VGPRs (seven wavefronts per SIMD, what the kernel's LDS allows anyway), no vector spills,
no scratch. When first built: lazy 63 VGPRs / 17 parked scalars, eager 65 / 2 (profiles/ec_lazy_protect.md)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

PROBE = ('#include "msdf_kernels.hpp"\nusing namespace msdfhip;\n'
         "template __global__ void msdfhip::k_ec_fast<3, %s>(BatchView, const MsdfHipGlyph *, int, int, int, int, const float *, float *, uint8_t *, MsdfHipConfig, "
         "const EcGlyphParams *, EcCandidate *, unsigned, int, const int *);\n")


def resources(lazy, tmp):
    from msdfgen_amd import build as B
    src = os.path.join(str(tmp), "probe_%s.hip" % lazy)
    with open(src, "w") as f:
        f.write(PROBE % lazy)
    flags = [f for f in B.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([B.hipcc()]+flags+["-I", B.CSRC, "-I", os.path.join(ROOT, "include"), "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        src, "-o", os.path.join(str(tmp), "probe_%s.o" % lazy)], capture_output=True, text=True, cwd=str(tmp))
    assert r.returncode == 0, r.stderr[-3000:]
    mine = r.stderr[r.stderr.index("Function Name: _ZN7msdfhip9k_ec_fast"):]
    res = {}
    for line in mine.splitlines()[1:]:
        if "Function Name:" in line:
            break
        m = re.search(r"\b(VGPRs Spill|SGPRs Spill|VGPRs|Occupancy|ScratchSize)\b[^:\n]*: (\d+)", line)
        if m:
            res[m.group(1)] = m.group(2)
    return res


@pytest.mark.parametrize("lazy", ["true", "false"])
def test_k_ec_fast_keeps_seven_wavefronts_without_vector_spills(lazy, tmp_path):
    res = resources(lazy, tmp_path)
    assert int(res["VGPRs"]) <= 72, res
    assert int(res["Occupancy"]) >= 7, res
    assert int(res["VGPRs Spill"]) == 0 and int(res["ScratchSize"]) == 0, res
    assert int(res["SGPRs Spill"]) <= 32, res                 # parked in the lanes of ONE vector register at most
