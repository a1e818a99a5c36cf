"""Stage 1 of the error-correction sweep as a mask of surviving tests per texel, appended once per tile (msdf_ec_fast.hpp: texelCandidateMask,
texelProtectMask, ecAppendItems) without a GPU.

tests/ec_emit_mask_host is a stand-alone program compiled from the product headers.

* The masks, over the 116 fields of tests/test_ec_hw_median_host.py (the special-value fields of tests/ecwordscases.py, finite wave fields, zeros, denormals,
  values at the vote's bound): texelCandidateMask equals the set of (k, j) that a per-test spelling emits -- one `if` per test, the predicates of the form
  the masks replaced, written out in the program; texelCandidatePairs emits them in that spelling's order; the same for the protect mask under the radii of
  the ten configurations used there (and two stretched transforms); texelFindFast returns the verdicts and the ordered candidates of a walk over the
  per-test spelling's items.
* The append: for 64 masks the written queue is exactly the multiset of expected items, no slot written twice, none beyond the count, the count the sum of
  the popcounts -- all masks zero, one lane only, all 24 (8) bits in all 64 lanes (the queue filled to its capacity), seeded random masks with the lanes
  reserving in a seeded order; a mask with bits that are no test writes its tests only."""
import pytest

import ecemitmaskcases as E


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return E.build_host(tmp_path_factory.mktemp("ec_emit_mask_host"))


@pytest.fixture(scope="module")
def cases():
    return E.host_cases()


def test_masks_equal_the_per_test_spelling(exe, cases, tmp_path):
    status, r = E.run_masks(exe, cases, tmp_path)
    print(r)
    assert len(cases) == 116
    assert r["cases"] == len(cases) and r["texels"] == sum(c["w"]*c["h"] for c in cases)
    assert r["bad_mask"] == 0 and r["bad_bits"] == 0 and r["bad_order"] == 0, r
    assert r["bad_protect"] == 0 and r["bad_protect_order"] == 0, r
    assert r["bad_find"] == 0, r
    assert r["bad_vote_mask"] == 0 and 0 < r["vote_texels"] < r["texels"], r      # min3 / max3 behind the vote: the same masks
    assert status == 0
    # not vacuous: every one of the 24 tests survives somewhere and bit 4*k+3 never does; texels with many survivors and with none; every protect pair
    tests = r["tests"]
    assert all((tests[b] > 50) == (b % 4 != 3) and (tests[b] == 0) == (b % 4 == 3) for b in range(32)), tests
    assert sum(tests) == r["survivors"] and r["full_texels"] > 100 and r["empty_texels"] > 100, r
    assert r["protect_comparisons"] == 12*r["texels"] and r["protect_pairs"] > r["texels"], r
    assert all((n > 100) == (m != 4) and (n == 0) == (m == 4) for m, n in enumerate(r["protect_bits"])), r
    assert r["find_comparisons"] == 10*r["texels"] and r["candidates"] > 100 and min(r["verdict_bits"]) >= 1, r


def test_append_writes_each_item_once(exe):
    status, r = E.run(exe, ["append", 20262, 600])
    print(r)
    assert status == 0, r
    assert r["find_capacity"] == 64*24 and r["protect_capacity"] == 64*8
    for q in ("find", "protect", "stray"):
        assert r[q]["bad"] == 0 and r[q]["items"] > 0, r
    assert r["find"]["rounds"] == 1+2*64+1+600 and r["protect"]["rounds"] == 1+64+1+600, r
    assert r["find"]["full_rounds"] == 1 and r["protect"]["full_rounds"] == 1, r           # all bits in all lanes: the queue is full, and holds it
    assert r["stray"]["full_rounds"] == 2, r                                               # a mask of 32 set bits takes the tests' slots, no more


def test_gpu_fields_hold_what_their_names_say(exe, tmp_path):
    """The fields of tests/test_gpu_ec_emit_mask.py, counted by the per-test spelling: no survivor in a constant field, survivors at exactly one texel of a
    one-texel field, and the noise fields are the densest."""
    gpu = E.gpu_cases()

    def count(names):
        packed = [{"w": gpu[n].shape[1], "h": gpu[n].shape[0], "field": gpu[n]} for n in names]
        status, r = E.run_masks(exe, packed, tmp_path, "gpu_fields.bin")
        assert status == 0, r
        return r

    assert sorted({n.split("_%dx%d_" % E.GPU_SIZES[0])[0] for n in gpu if "16x16" in n}) == sorted(E.KINDS)
    r = count([n for n in gpu if n.startswith("constant_")])
    assert r["survivors"] == 0 and r["empty_texels"] == r["texels"], r
    for n in gpu:
        if n.startswith("one_texel_"):
            r = count([n])
            assert r["empty_texels"] == r["texels"]-1 and r["survivors"] >= 8, (n, r)
    noise = count([n for n in gpu if n.startswith("noise_")])
    wave = count([n for n in gpu if n.startswith("wave_")])
    print("survivors per texel: noise %.2f, waves %.2f" % (noise["survivors"]/noise["texels"], wave["survivors"]/wave["texels"]))
    # (a test survives only at the texel of its pair that lies farther from the edge, so about half of the 24 is the most a field can average: the noise
    # fields put several hundred items into a tile's queue of 1536, the one-texel fields eight, the constant ones none)
    assert noise["survivors"]/noise["texels"] > wave["survivors"]/wave["texels"] > 0, (noise, wave)
    assert noise["survivors"] > 6*noise["texels"] and noise["full_texels"] > 0, noise


def test_sanitized_build_of_the_host_program(cases, tmp_path_factory):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, run as it is), over a quarter of the fields and the whole
    append. Skipped only where an EMPTY program cannot be built with those flags; any failure of the real build or run fails the test."""
    import os
    import subprocess
    tmp = tmp_path_factory.mktemp("ec_emit_mask_host_san")
    src, probe = os.path.join(str(tmp), "probe.cpp"), os.path.join(str(tmp), "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    b = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", probe, src], capture_output=True)
    if b.returncode != 0 or subprocess.run([probe], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    san = E.build_host(tmp, sanitize=True)
    status, r = E.run(san, ["append", 7, 200])
    assert status == 0, r
    status, r = E.run_masks(san, cases[::4], tmp)
    assert status == 0 and r["cases"] == len(cases[::4]), r
