"""k_ec_fast behind its finiteness vote (msdf_kernels.hpp: ecFastBody -- hardware median, indexed channel reads, folded lazy configuration) on the device.

Arbitrary fields go through the shapeless entries (msdfhip_error_correction_shapeless: k_ec_fast on the field as it is; the entry returns no stencil, so
the corrected field is what is compared) and must equal the host walk ecTexelFast of the same headers, which keeps the exact median, bit for bit:
16x16 and 10x10 fields of one glyph = four tiles (10x10: partial tiles on two sides) -- seeded plane waves; the same with one -inf texel that one, two or
all four tiles hold or see in their halo, so that wavefronts of ONE launch take different paths; with two -inf channels in one texel (their difference is
a NaN); with +-0, denormals and a channel just below the vote's bound, and with one just above it. Four fields, two of them with a -inf texel,
corrected by four host threads at once behind one leader slot (the calls that queue up are merged into one batch of several glyphs: the flag is per
wavefront, not per launch). And two real glyphs, the smallest two-contour shape of tests/golden/latin.npz first, through GlyphBatch.generate at msdf
16x16 under the default configuration (the lazy instantiation, with its distance-check candidates) against the oracle, tiles and stencil.

Every device call is made by ONE child process (tests/echwmed_gpu_child.py) under a time limit of its own; this process never opens the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal
import echwmedcases as H
import echwmed_gpu_child as child
import ecwordscases as W

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 240          # seconds; the child needs a few


@pytest.fixture(scope="module")
def device(tmp_path_factory):
    """What the child computed on the GPU. A child that faults, hangs into its limit or returns non-zero fails every test here."""
    out = os.path.join(str(tmp_path_factory.mktemp("ec_hwmed_gpu")), "device.npz")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable]+flags+[child.__file__, out], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    print(r.stdout[-300:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """name, p -> the host walk's corrected field, computed once."""
    tmp = tmp_path_factory.mktemp("ec_hwmed_host")
    cases = H.gpu_cases()
    names = list(cases)
    packed = [{"w": cases[n].shape[1], "h": cases[n].shape[0], "field": cases[n], "protect_all": p, "ratio": W.RATIOS[0]} for n in names for p in (0, 1)]
    res = H.run_correct(H.build_host(tmp), packed, tmp)
    return cases, {(n, p): res[2*i+p] for i, n in enumerate(names) for p in (0, 1)}


def same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


@pytest.mark.parametrize("kind", ["wave", "neginf_corner", "neginf_inner", "neginf_edge", "nan_difference", "zeros_bound", "zeros_above_bound"])
@pytest.mark.parametrize("w,h", H.GPU_SIZES)
def test_shapeless_sweep_equals_the_host_walk(device, host, kind, w, h):
    cases, want = host
    names = [n for n in cases if n.startswith("%s_%dx%d_" % (kind, w, h))]
    assert len(names) == 3
    changed = 0
    for n in names:
        for p in (0, 1):
            got = device["shapeless_%s_%d" % (n, p)]
            assert got.shape == want[(n, p)].shape == (h, w, 3)
            assert same_bits(got, want[(n, p)]), (n, p, int((got.view(np.uint32) != want[(n, p)].view(np.uint32)).sum()))
            changed += not same_bits(got, cases[n])
    assert changed >= 1                                              # (the comparison is not between untouched fields)


def test_fields_hold_what_the_cases_say():
    cases = H.gpu_cases()
    for (w, h) in H.GPU_SIZES:
        f = cases["neginf_edge_%dx%d_0" % (w, h)]
        assert np.isneginf(f).sum() == 1 and np.isneginf(f[3, 7, 1])              # tiles 0 and 1 hold / see it, rows 7.. (tiles 2 and 3) do not
        f = cases["nan_difference_%dx%d_0" % (w, h)]
        with np.errstate(invalid="ignore"):
            assert np.isnan(f[3, 7, 1]-f[3, 7, 0])
        f = cases["zeros_bound_%dx%d_0" % (w, h)]
        assert (np.abs(f) < H.BOUND).all() and (np.abs(f) == H.BELOW).sum() >= 4 and np.signbit(f[f == 0]).any() and (~np.signbit(f[f == 0])).any()
        assert ((f != 0) & (np.abs(f) < np.finfo(np.float32).tiny)).any()
        f = cases["zeros_above_bound_%dx%d_0" % (w, h)]
        assert (np.abs(f) == H.ABOVE).sum() == 1


def test_fields_corrected_at_once(device, host):
    _, want = host
    print("largest concurrent batch:", int(device["pair_largest"]))
    for r in range(child.PAIR_ROUNDS):
        for k, n in enumerate(child.PAIR_FIELDS):
            assert same_bits(device["pair_%d_%d" % (r, k)], want[(n, 0)]), (r, n)


def test_two_real_glyphs_equal_the_oracle(device, oracle):
    sub, bounds = child.fixture()
    assert sub.n_glyphs == 2
    xfs = child.frames(bounds)
    s = child.GLYPH_SIZE
    want = np.zeros((2, s, s, 3), np.float32)
    want_st = np.zeros((2, s, s), np.uint8)
    for g in range(2):
        want[g] = oracle.generate(sub.shape(g), 3, s, s, xfs[g], stencil=want_st[g])
    assert_bit_equal(device["tiles"], want, "tiles")
    assert (device["stencil"] == want_st).all()
