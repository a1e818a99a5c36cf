"""The hardware median of the error-correction sweep (msdf_device.hpp: med3f, medianOf; the HWMED / INDEXED / CORDER switches of msdf_ec_fast.hpp) without a GPU.

tests/ec_hw_median_host is a stand-alone program compiled from the product headers; on the host med3f runs the ISA's definition of v_med3_f32.

* The median: over all triples of special values (+-0, +-denormal min / max, +-FLT_MIN, +-1, .5 and its neighbours, +-FLT_MAX, +-inf) and four million
  seeded random triples, every triple without a NaN gives the same VALUE by both spellings. What the program reports and this test does not judge equal:
  results that differ in the sign of a zero, and triples with a NaN -- the two facts behind the kernel's vote and behind the apply step keeping medianf.
* The sweep: texelFindFast<HWMED> against texelFindFast<> under every (mode, distance check, order, protection) combination, and evaluatePair as
  k_ec_fast compiles it (hardware median, indexed channel reads, the lazy orders' configuration folded) against the plain call, item by item; the
  deviation and the protectEdges pairs of the lazy protection round likewise. Over the special-value fields of tests/ecwordscases.py, finite wave fields,
  fields of zeros, denormals and values next to the vote's bound, and fields whose every channel is at the bound. At every texel where the vote passes the
  verdict bits and the ordered candidate lists are identical."""
import pytest

import echwmedcases as H


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return H.build_host(tmp_path_factory.mktemp("ec_hw_median_host"))


@pytest.fixture(scope="module")
def cases():
    return H.host_cases()


def test_hardware_median_equals_medianf_on_every_triple_without_nan(exe):
    status, r = H.run(exe, ["median", 20261, 4000000])
    print(r)
    assert r["special_triples"] == 17**3 and r["random_triples"] == 4000000
    assert r["special_value_mismatch"] == 0 and r["random_value_mismatch"] == 0, r
    assert status == 0
    # reported, not judged: why the apply step keeps medianf, and why the kernel votes
    assert r["special_zero_sign_differs"] > 0 and r["nan_differs"] > 0 and r["random_nan_triples"] > 0, r


def test_sweep_is_identical_where_the_vote_passes(exe, cases, tmp_path):
    status, r = H.run_sweep(exe, cases, tmp_path)
    print(r)
    assert r["cases"] == len(cases) and r["texels"] == sum(c["w"]*c["h"] for c in cases)
    assert r["bad"] == 0 and r["bad_folded"] == 0 and r["bad_protect"] == 0 and r["bad_deviation"] == 0, r
    assert status == 0
    # not vacuous: texels of both kinds, items of both kinds, every verdict bit and candidates behind the vote
    assert 0 < r["vote_texels"] < r["texels"]
    assert r["linear_items"] > 1000 and r["diagonal_items"] > 1000 and r["candidates"] > 100, r
    assert min(r["verdict_bits"]) >= 1, r
    assert r["folded_comparisons"] >= 10*r["items"] and r["protect_comparisons"] > r["vote_texels"], r
    # the reason for the vote: where it fails, the two instantiations do differ somewhere
    assert r["differ_outside_vote"] > 0, r


def test_fields_at_the_bound_pass_the_vote(exe, tmp_path):
    """Every channel just below 2^100 in magnitude: all texels vote in favour and nothing overflows into a NaN -- the instantiations agree."""
    fields = [{"w": 9, "h": 9, "field": H.bound_field(9, 9, s)} for s in range(8)]
    status, r = H.run_sweep(exe, fields, tmp_path, "bound.bin")
    assert status == 0 and r["vote_texels"] == r["texels"] == 8*81 and r["items"] > 0, r
    above = [dict(c, field=H.with_texel(c["field"], 4, 4, (H.BOUND, 0., 0.))) for c in fields]
    status, r = H.run_sweep(exe, above, tmp_path, "above.bin")
    assert status == 0 and r["vote_texels"] == 8*(81-9), r            # 2^100 itself is turned away, with its eight neighbours


def test_sanitized_build_of_the_host_program(cases, tmp_path_factory):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only), over a quarter of the fields. Skipped only where an EMPTY
    program cannot be built with those flags; any failure of the real build or run fails the test."""
    import os
    import subprocess
    tmp = tmp_path_factory.mktemp("ec_hw_median_host_san")
    src, probe = os.path.join(str(tmp), "probe.cpp"), os.path.join(str(tmp), "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    b = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", probe, src], capture_output=True)
    if b.returncode != 0 or subprocess.run([probe], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    san = H.build_host(tmp, sanitize=True)
    status, r = H.run(san, ["median", 7, 200000])
    assert status == 0, r
    status, r = H.run_sweep(san, cases[::4], tmp)
    assert status == 0 and r["cases"] == len(cases[::4]), r
