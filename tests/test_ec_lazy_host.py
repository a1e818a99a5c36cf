"""The lazy protection order of the error-correction sweep (msdf_ec_fast.hpp: ecLazyProtect, ecTexelFast -- the host walk of k_ec_fast) without a GPU.

tests/ec_lazy_host is a stand-alone program compiled from the product headers. For every texel of every input, under all nine Mode x DistanceCheckMode
combinations and both flips, it compares the stencil byte of the lazy and of the eager walk (their deferred candidates judged by ecEvaluateCandidate) with the
per-texel pipeline ecTexelStencil of msdf_ec.hpp, the raw byte and the deferred-candidate set of the two walks with each other, and the new verdict bit with
the oracle's base pass run twice (protectedFlag false / true). It exits with 1 on any difference and prints the counts asserted below.

Inputs: pre-correction fields of 40 Basic-Latin fixture glyphs at 16x16 and 23x17 (range 2 texels), and seeded plane-wave fields around .5
(eclazycases.random_cases). Counts of the kinds of texel the lazy order distinguishes, by the oracle's functions alone, as first counted on a CPU:
                                                   glyph fields (51 760 texels)   random fields (7 764 texels)
    conditional, then protected by an edge pair                    8                          732
    conditional, then protected by a corner                       38                           75
    conditional, left unprotected (-> ERROR)                    1 104                          147
    unconditional ERROR together with a conditional bit             6                          164      (from the first visit's verdict: no oracle has that bit)
    texels that hold a distance-check candidate back                2                           20
    ... and stay unprotected (the eager order hands the             0                            5
        candidate to nobody: without the hold-back the candidate sets of the two orders differ at exactly these texels)
"""
import os
import subprocess

import pytest

import eclazycases as E


@pytest.fixture(scope="module")
def cases(latin, oracle):
    batch, _, bounds = latin
    return E.glyph_cases(batch, bounds, oracle, E.HOST_SIZES)+E.random_cases(batch, bounds)


@pytest.fixture(scope="module")
def report(cases, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ec_lazy_host")
    return E.run_host(E.build_host(tmp), cases, tmp)


def test_inputs_are_the_ones_described(cases):
    assert len({c["glyph"] for c in cases if c["group"] == E.GROUP_GLYPHS}) == 40
    assert {(c["w"], c["h"]) for c in cases} == set(E.HOST_SIZES)
    for group in (E.GROUP_GLYPHS, E.GROUP_RANDOM):
        assert {c["flip"] for c in cases if c["group"] == group} == {0, 1}


def test_lazy_and_eager_walks_equal_the_per_texel_pipeline(report, cases):
    status, r = report
    assert r["cases"] == len(cases)
    assert r["texels_checked"] == 9*sum(c["w"]*c["h"] for c in cases)            # every Mode x DistanceCheckMode combination
    assert [tuple(row[:2]) for row in r["bad_by_config"]] == [(m, d) for m in E.MODES for d in E.DISTANCE_CHECKS]
    assert r["deferred_candidates"] > 1000                                          # the candidate sets compared are not empty
    for key in ("bad_lazy_stencil", "bad_eager_stencil", "bad_raw_byte", "bad_candidate_set", "bad_conditional_bit"):
        assert r[key] == 0, (key, r[key], r["bad_by_config"])
    assert status == 0


def test_every_kind_of_texel_occurs(report):
    """Not vacuous: both groups of inputs hold conditional texels that an edge pair protects, that a corner protects, that stay unprotected and become
    ERROR, and texels with an unconditional ERROR next to a conditional bit; some texels hold a distance-check candidate back behind a conditional artifact,
    and of those in the random fields some turn out protected and some do not."""
    _, r = report
    for group in (E.GROUP_GLYPHS, E.GROUP_RANDOM):
        for kind in E.KINDS:
            assert r["groups"][group][kind] >= 1, (group, kind, r["groups"][group])
        assert r["groups"][group]["held_back"] >= 1, r["groups"][group]
    rnd = r["groups"][E.GROUP_RANDOM]
    assert 1 <= rnd["held_back_unprotected"] < rnd["held_back"], rnd                # held back and then dropped, held back and then handed over
    assert sum(rnd[k] for k in E.KINDS) >= rnd["texels"]//20                        # "common" in the random fields: one texel in twenty at least
    # the lazy order resolves the protection of a small share of the texels and queues a small share of the eager order's pairs
    g = r["groups"][E.GROUP_GLYPHS]
    conditional = sum(g[k] for k in E.KINDS[:3])
    assert conditional <= g["texels_resolved"] <= conditional+g["held_back"]       # (a held-back candidate asks for the protection whatever the verdict)
    assert g["texels_resolved"] < g["texels"]//20
    assert 0 < g["lazy_protect_items"] < g["eager_protect_items"]//20


def _sanitizers_link(tmp):
    """Can g++ compile, link and run an empty program with -fsanitize=address,undefined here (are the sanitizer runtimes installed)?"""
    src, exe = os.path.join(str(tmp), "probe.cpp"), os.path.join(str(tmp), "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", exe, src], capture_output=True)
    return r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


def test_sanitized_build_of_the_host_program(cases, tmp_path_factory):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only), over a fifth of the inputs. Skipped only where an EMPTY
    program cannot be built with those flags; any failure of the real build or run fails the test."""
    tmp = tmp_path_factory.mktemp("ec_lazy_host_san")
    if not _sanitizers_link(tmp):
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    exe = E.build_host(tmp, sanitize=True)
    status, r = E.run_host(exe, cases[::5], tmp)
    assert status == 0 and r["cases"] == len(cases[::5])
