"""The wedge flags of the distance walk without a GPU (tests/wedge_flags_host, compiled from the product headers; shapes: tests/wedgecases.py).

Phase 1 of k_distance decides per (tile, edge end) whether the whole tile lies outside the wedge in which the reference lets that end contribute a
perpendicular distance (msdf_cull.hpp: cullWedgeOutside); a survivor carries the two bits in its list entry and the per-texel walk leaves a flagged end out
(msdf_device.hpp: selEdgeRelevantWedges, selAddEdge). Over the Latin set, CJK-like shapes and crafted outlines (needle corners, corners at a tile's centre
and where four tiles meet, zero-length end tangents, contours far outside the bitmap), at 8 x 8, 16 x 16 and 64 x 64, autoframed, mirrored and 1:8
anisotropic, both combiners, SEL 2, 3 and 4, for every tile:

* a set bit, of any edge of the glyph, means that no texel of the tile passes that end's domain test as selAddEdge evaluates it;
* the lockstep walk with the bits leaves every lane's selector bitwise equal to the walk without them after every contour, with the same votes.

The program also walks with BOTH bits forced on for every survivor: that walk must differ, or the comparison would prove nothing."""
import pytest

import wedgecases as W


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return W.build_host(tmp_path_factory.mktemp("wedge_flags_host"))


def check(status, r, n_cases):
    assert r["cases"] == n_cases, r
    for combo in W.COMBOS:
        n = r[combo]
        assert n["domain_violations"] == 0 and n["selector_mismatches"] == 0 and n["vote_mismatches"] == 0, (combo, n)
        assert n["lanes_compared"] > 0 and n["bits_checked"] >= n["bits_set"] > 0, (combo, n)
    assert status == 0, r


def not_vacuous(r):
    for combo in W.COMBOS:
        n = r[combo]
        assert n["wedge_outside_both"] > 0 and n["wedge_outside_one"] > 0 and n["ends_outside"] > 0 and n["both_ends_outside"] > 0, (combo, n)
        assert n["ends_outside"] < 2*n["evaluated"], (combo, n)                       # and ends that are NOT flagged are evaluated too
        assert n["forced_mismatches"] > 0, (combo, n)                                 # forcing the bits on changes selectors: the comparison can fail


def test_crafted_outlines(exe, tmp_path):
    cases = W.crafted_cases(W.SIZES)
    status, r = W.run(exe, cases, tmp_path)
    print(r)
    check(status, r, len(cases))
    not_vacuous(r)
    assert r["zero_direction_edges"] > 0, r                                           # REC_A_ZERO / REC_B_ZERO records are among them


@pytest.mark.parametrize("size", W.SIZES, ids=lambda s: "%dx%d" % s)
def test_latin_set(exe, tmp_path, size):
    cases = W.latin_cases((size,))
    assert len(cases) == 2*94
    status, r = W.run(exe, cases, tmp_path)
    print({c: W.per_tile(r, c) for c in W.COMBOS})
    check(status, r, len(cases))
    not_vacuous(r)


def test_cjk_like_shapes(exe, tmp_path):
    cases = W.cjk_cases()
    status, r = W.run(exe, cases, tmp_path)
    print({c: W.per_tile(r, c) for c in W.COMBOS})
    check(status, r, len(cases))
    not_vacuous(r)


def test_benchmark_sample_counts(exe, tmp_path):
    """Every 41st glyph of the benchmark's set at its size: the per-tile counts that say what the flags can save (printed; profiles/wedge_flags.md quotes
    them). Most tests that reach the wedge stage find the tile outside both wedges, and most ends of evaluated edges are flagged."""
    cases = W.bench_sample()
    assert len(cases) == 200
    status, r = W.run(exe, cases, tmp_path)
    for c in W.COMBOS:
        print(c, {k: round(v, 2) for k, v in W.per_tile(r, c).items()})
    check(status, r, len(cases))
    n = r["overlap_sel3"]
    assert 2*n["wedge_outside_both"] > n["wedge_stage"] and n["ends_outside"] > n["evaluated"], n      # more than half of the tests / of the 2 ends per edge


def test_sanitized_build_of_the_host_program(tmp_path_factory):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only, run as it is) over the crafted outlines at the two small
    sizes and a tenth of the Latin set. Skipped only where an EMPTY program cannot be built with those flags."""
    import os
    import subprocess
    tmp = tmp_path_factory.mktemp("wedge_flags_host_san")
    src, probe = os.path.join(str(tmp), "probe.cpp"), os.path.join(str(tmp), "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    b = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", probe, src], capture_output=True)
    if b.returncode != 0 or subprocess.run([probe], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    san = W.build_host(tmp, sanitize=True)
    cases = W.crafted_cases(W.SIZES[:2])+W.latin_cases(W.SIZES[:2], step=10)
    status, r = W.run(san, cases, tmp)
    check(status, r, len(cases))
