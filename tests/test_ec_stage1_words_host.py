"""Stage 1 of the error-correction sweep from per-texel class words (msdf_ec_fast.hpp: ecTexelClassWord, loadNeighbourhood, texelCandidatePairs) without a GPU.

tests/ec_stage1_words_host is a stand-alone program compiled from the product headers. For every texel of every input it compares the set of (neighbour,
channel pair) tests the word-based stage 1 emits, and the inside bits of the texel's neighbourhood, with the stage 1 of the commit before -- kept in the
program word for word: every value derived from the channels and the coordinates, nothing shared between texels. Queue order was never part of the result
(the kernel pushes with an LDS atomic, verdicts are an OR), so equal sets mean an equal sweep.

Inputs: the pre-correction fields of tests/eclazycases.py (40 Basic-Latin fixture glyphs at 16x16 and 23x17, both row orders; the seeded plane-wave fields),
and crafted fields (tests/ecwordscases.py) of 1x1, 1x9, 9x1, 2x2, 8x8, 9x9 and 10x17 texels, seeded with equal channels, +0 / -0 and denormal channel
differences, +-inf and NaN."""
import numpy as np
import pytest

import eclazycases as E
import ecwordscases as W


@pytest.fixture(scope="module")
def lazy_cases(latin, oracle):
    batch, _, bounds = latin
    return E.glyph_cases(batch, bounds, oracle, E.HOST_SIZES)+E.random_cases(batch, bounds)


@pytest.fixture(scope="module")
def crafted():
    return W.crafted_cases()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return W.build_host(tmp_path_factory.mktemp("ec_stage1_words_host"))


def test_inputs_are_the_ones_described(lazy_cases, crafted):
    assert len({c["glyph"] for c in lazy_cases if c["group"] == E.GROUP_GLYPHS}) == 40
    assert {(c["w"], c["h"]) for c in lazy_cases} == set(E.HOST_SIZES)
    for group in (E.GROUP_GLYPHS, E.GROUP_RANDOM):
        assert {c["flip"] for c in lazy_cases if c["group"] == group} == {0, 1}
    assert {(c["w"], c["h"]) for c in crafted} == set(W.CRAFTED_SIZES)
    for (w, h) in W.CRAFTED_SIZES:                                                  # every size holds every kind of special texel
        n = W.census([c["field"] for c in crafted if (c["w"], c["h"]) == (w, h)])
        assert all(n[k] >= 1 for k in W.KINDS), ((w, h), n)
    assert W.census([c["field"] for c in lazy_cases])["nan"] == 0                   # (the glyph and plane-wave fields are finite)


def test_word_based_stage_1_emits_the_same_tests(exe, lazy_cases, crafted, tmp_path):
    cases = lazy_cases+crafted
    status, r = W.run_compare(exe, cases, tmp_path)
    print(r)
    assert r["cases"] == len(cases) and r["texels_compared"] == sum(c["w"]*c["h"] for c in cases)
    assert r["bad_test_set"] == 0 and r["bad_test_count"] == 0 and r["bad_valid_mask"] == 0, r
    assert status == 0
    # not vacuous: every one of the 24 tests (8 neighbours x 3 channel pairs) is emitted, and texels of all 16 border patterns were compared
    assert len(r["emitted"]) == 24 and min(r["emitted"]) >= 1, r["emitted"]
    assert len(r["border_patterns"]) == 16 and min(r["border_patterns"]) >= 1, r["border_patterns"]


def test_crafted_fields_alone_reach_every_test_and_border(exe, crafted, tmp_path):
    """The special texels do not silence stage 1: on the crafted fields alone every test is emitted and every border pattern occurs."""
    status, r = W.run_compare(exe, crafted, tmp_path)
    assert status == 0, r
    assert min(r["emitted"]) >= 1 and min(r["border_patterns"]) >= 1, r


def test_class_word_layout(exe, tmp_path):
    """The word of a single texel, read back through the classifier's inside mask: a 1x1 field has exactly its centre inside; and a texel whose
    differences are NaN emits nothing against any neighbour (no sign bit set), on a 3x3 field of NaN texels around a finite one and the reverse."""
    one = {"w": 1, "h": 1, "field": np.full((1, 1, 3), .25, np.float32)}
    nan_ring = np.full((3, 3, 3), np.nan, np.float32)
    nan_ring[1, 1] = (.2, .6, .9)
    nan_centre = np.stack([np.full((3, 3), v, np.float32) for v in (.2, .6, .9)], -1)
    nan_centre[1, 1] = np.nan
    status, r = W.run_compare(exe, [one, {"w": 3, "h": 3, "field": nan_ring}, {"w": 3, "h": 3, "field": nan_centre}], tmp_path)
    assert status == 0 and r["texels_compared"] == 19, r


def test_sanitized_build_of_the_host_program(lazy_cases, crafted, tmp_path_factory):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only), over the crafted fields and a fifth of the others. Skipped
    only where an EMPTY program cannot be built with those flags; any failure of the real build or run fails the test."""
    import subprocess
    import os
    tmp = tmp_path_factory.mktemp("ec_stage1_words_host_san")
    src, probe = os.path.join(str(tmp), "probe.cpp"), os.path.join(str(tmp), "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    b = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", probe, src], capture_output=True)
    if b.returncode != 0 or subprocess.run([probe], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    san = W.build_host(tmp, sanitize=True)
    cases = crafted+lazy_cases[::5]
    status, r = W.run_compare(san, cases, tmp)
    assert status == 0 and r["cases"] == len(cases)
    shapeless = [dict(c, protect_all=i % 2) for i, c in enumerate(crafted)]
    assert len(W.run_correct(san, shapeless, tmp)) == len(shapeless)
