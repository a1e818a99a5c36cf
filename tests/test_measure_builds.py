"""The measurement builds of the kernels still compile and still write their tables (no GPU: hipcc cross-compiles one kernel in a few seconds).

msdf_measure.hpp gives every profiling hook of the kernels two forms: a real one under -DMSDF_PROFILE_WAITS / -DMSDF_PROFILE_QUERY and an empty one in
the build that ships. Nobody runs the first form day to day; this test keeps it from rotting unseen. It asserts nothing about instruction choice."""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")

K_DISTANCE = ("k_distance<3, true, false, 4>(int, const int32_t *, const int32_t *, const EdgeRec *, const int8_t *, const MsdfHipGlyph *, int, int, int, int, int, float *, int, "
              "unsigned, double *, size_t, const int *, int, unsigned *, unsigned)")
K_EC_QUERY = ("k_ec_query<3, true>(int, const int32_t *, const int32_t *, const EdgeRec *, const int8_t *, const MsdfHipGlyph *, int, int, const float *, float *, uint8_t *, "
              "MsdfHipConfig, const EcGlyphParams *, const EcCandidate *, unsigned, const int *, int *, int, int, int, EcQueryPolicy, unsigned *, const int *, int)")
TABLES = ("gWaitProfile", "gQueryProfile", "gQueryDetail")


def defines(asm, table):
    """the assembly holds the table's storage: a label of its (mangled) name"""
    return any(re.match(r"_ZN7msdfhip%d%sE:" % (len(table), table), l) for l in asm)


def writes(asm, table):
    """the kernel forms the table's address and issues 64-bit atomics to global memory (a guard against rot, not a proof: the reference to the table goes when its flush does)"""
    return any(re.search(r"_ZN7msdfhip%d%sE@rel32" % (len(table), table), l) for l in asm) and any(re.match(r"\s+global_atomic_\w+_x2\b", l) for l in asm)


@pytest.mark.parametrize("kernel,flag,tables", [(K_DISTANCE, "-DMSDF_PROFILE_WAITS", ("gWaitProfile",)),
                                                (K_EC_QUERY, "-DMSDF_PROFILE_QUERY=1", ("gQueryProfile", "gQueryDetail")),   # (the second: profQueryDone, the item histogram)
                                                (K_EC_QUERY, "-DMSDF_PROFILE_QUERY=2", ("gQueryProfile", "gQueryDetail"))])
def test_measurement_build_compiles_and_writes_its_table(kernel, flag, tables):
    from isa_loop_depth import compile_kernel
    asm, _ = compile_kernel(kernel, [flag])                # (raises with the compiler's message if the build does not compile)
    for table in tables:
        assert defines(asm, table), "%s: no definition of %s" % (flag, table)
        assert writes(asm, table), "%s: %s is never written" % (flag, table)


@pytest.mark.parametrize("kernel", [K_DISTANCE, K_EC_QUERY], ids=["k_distance", "k_ec_query"])
def test_regular_build_has_no_table(kernel):
    from isa_loop_depth import compile_kernel
    asm, _ = compile_kernel(kernel)
    assert not any(t in l for l in asm for t in TABLES)
