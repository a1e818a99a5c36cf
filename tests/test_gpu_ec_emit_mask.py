"""k_ec_fast's stage 1 as a mask of surviving tests per texel, appended to the item queue once per tile (msdf_kernels.hpp: ecFastBody, ecAppendWave;
msdf_ec_fast.hpp: texelCandidateMask, texelProtectMask, ecAppendItems) on the device.

Fields of 16x16 and 10x10 (one glyph = four 8x8 tiles; 10x10: partial tiles on two sides) go through both shapeless entries (k_ec_fast on the field as it is;
the entries return the corrected field and no stencil) and must equal the host walk ecTexelFast of the same headers bit for bit: a constant field, where
no test survives and every queue stays empty; seeded noise in [0, 1], the densest queues; a field in which exactly one texel has survivors; plane waves;
a field with a -inf texel, where the finiteness vote fails in all four tiles or in one. And two real glyphs at msdf 16x16 under the default configuration
(lazy order, with distance-check candidates) and under EDGE_PRIORITY without the distance check (eager order: protect queue and find queue filled in one
phase A) against the oracle, tiles and stencil. The order in which distance-check candidates reach a glyph's segment is free, and the segment is not
handed out: what is compared is their number per glyph against the host walk's, and the verdicts they lead to (the stencil).

Every device call is made by ONE child process (tests/ecemitmask_gpu_child.py) under a time limit of its own; this process never opens the GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal
import ecemitmask_gpu_child as child
import ecemitmaskcases as E
import echwmed_gpu_child as G
import echwmedcases as H
import ecwordscases as W

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 240          # seconds; the child needs a few


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """What the child computed on the GPU. A child that faults, hangs into its limit or returns non-zero fails every test here."""
    out = os.path.join(str(tmp_path_factory.mktemp("ec_emit_mask_gpu")), "device.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable]+flags+[child.__file__, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout[-300:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """name, p -> the host walk's corrected field, computed once."""
    tmp = tmp_path_factory.mktemp("ec_emit_mask_host_walk")
    cases = E.gpu_cases()
    names = list(cases)
    packed = [{"w": cases[n].shape[1], "h": cases[n].shape[0], "field": cases[n], "protect_all": p, "ratio": W.RATIOS[0]} for n in names for p in (0, 1)]
    res = H.run_correct(H.build_host(tmp), packed, tmp)
    return cases, {(n, p): res[2*i+p] for i, n in enumerate(names) for p in (0, 1)}


def same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


@pytest.mark.parametrize("kind", E.KINDS)
@pytest.mark.parametrize("w,h", E.GPU_SIZES)
def test_shapeless_sweep_equals_the_host_walk(device, host, kind, w, h):
    cases, want = host
    names = [n for n in cases if n.startswith("%s_%dx%d_" % (kind, w, h))]
    assert len(names) == 2
    changed = 0
    for n in names:
        for p in (0, 1):
            got = device["shapeless_%s_%d" % (n, p)]
            assert got.shape == want[(n, p)].shape == (h, w, 3)
            assert same_bits(got, want[(n, p)]), (n, p, int((got.view(np.uint32) != want[(n, p)].view(np.uint32)).sum()))
            changed += not same_bits(got, cases[n])
    print(kind, w, h, "fields changed by the correction:", changed)
    if kind == "constant":
        assert changed == 0                                          # nothing survives stage 1: nothing to correct
    elif kind != "one_texel":
        assert changed >= 1                                          # (the comparison is not between untouched fields)


def test_fields_hold_what_the_cases_say():
    cases = E.gpu_cases()
    assert len(cases) == 2*2*len(E.KINDS)
    for (w, h) in E.GPU_SIZES:
        tag = "%dx%d" % (w, h)
        for s in range(2):
            f = cases["constant_%s_%d" % (tag, s)]
            assert (f == f[0, 0, 0]).all()
            f = cases["noise_%s_%d" % (tag, s)]
            assert f.min() >= 0 and f.max() <= 1 and len(np.unique(f)) > f.size//2
            f = cases["one_texel_%s_%d" % (tag, s)]
            assert ((f != f[0, 0]).any(-1)).sum() == 1
        assert np.isneginf(cases["neginf_%s_0" % tag][7, 7, 0]) and np.isneginf(cases["neginf_%s_0" % tag]).sum() == 1
        assert np.isneginf(cases["neginf_%s_1" % tag][2, 2, 1]) and np.isneginf(cases["neginf_%s_1" % tag]).sum() == 1


@pytest.mark.parametrize("c,ec_dist", [(0, 1), (1, 0)])
def test_two_real_glyphs_equal_the_oracle(device, oracle, c, ec_dist):
    sub, bounds = G.fixture()
    assert sub.n_glyphs == 2
    xfs = G.frames(bounds)
    s = G.GLYPH_SIZE
    want = np.zeros((2, s, s, 3), np.float32)
    want_st = np.zeros((2, s, s), np.uint8)
    for g in range(2):
        want[g] = oracle.generate(sub.shape(g), 3, s, s, xfs[g], ec_dist=ec_dist, stencil=want_st[g])
    assert_bit_equal(device["tiles_%d" % c], want, "tiles")
    assert (device["stencil_%d" % c] == want_st).all()


def test_distance_check_candidates_are_those_of_the_host_walk(device):
    """The default configuration: as many candidates per glyph as the host walk hands to its sink (their order in the segment is free), no overflow."""
    import emu
    e = emu.Emu(lean=True)
    e.lib.emu_last_deferred.restype = C.c_long
    sub, bounds = G.fixture()
    xfs = G.frames(bounds)
    s = G.GLYPH_SIZE
    counts = device["counts_0"]
    assert counts[0] == 0
    want = []
    for g in range(2):
        e.generate(sub.shape(g), 3, s, s, xfs[g])
        want.append(int(e.lib.emu_last_deferred()))
    print("distance-check candidates per glyph:", want)
    assert [int(n) for n in counts[1:]] == want and sum(want) > 0
