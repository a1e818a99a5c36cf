"""The diagonal artifact test of the error-correction sweep with in-range roots and extrema first (msdf_ec_fast.hpp: diagonalPairFast, diagonalRootsInRange)
without a GPU.

tests/ec_roots_host is a stand-alone program compiled from the product headers. For every texel of every input and each of its diagonal (neighbour, channel
pair) tests -- a superset of the items stage 1 queues -- it compares the verdict bits and the ordered list of sink(t) values, bitwise, of evaluatePair with
the diagonalPairFast of the commit before, kept in the program word for word, under EC_ORDER_EAGER (texel unprotected and protected), EC_ORDER_LAZY and
EC_ORDER_LAZY_HELD; and of an emulation of the dense form (one lane per (item, root, test) unit, chunks of 64) written with the same helpers.

Inputs: the pre-correction fields of tests/eclazycases.py (40 Basic-Latin fixture glyphs at 16x16 and 23x17, both row orders; the seeded plane-wave fields),
every 512th glyph of tests/golden/dejavu8192.npz at 64x64, the crafted 2x2 cells of tests/ecrootscases.py in 8x8 and 9x9 fields, the crafted fields of
tests/ecwordscases.py (equal channels, +-0, denormal differences, +-inf, NaN) and further seeded plane-wave fields, which the bars below need."""
import pytest

import eclazycases as E
import ecrootscases as R
import ecwordscases as W


@pytest.fixture(scope="module")
def cases(latin, oracle):
    batch, _, bounds = latin
    words = [dict(c, group=R.GROUP_CRAFTED) for c in W.crafted_cases() if (c["w"], c["h"]) in ((8, 8), (9, 9), (10, 17))]
    return E.glyph_cases(batch, bounds, oracle, E.HOST_SIZES)+E.random_cases(batch, bounds)+R.bench_cases(oracle, 512)+R.crafted_cases()+words+R.extra_cases()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return R.build_host(tmp_path_factory.mktemp("ec_roots_host"))


@pytest.fixture(scope="module")
def report(exe, cases, tmp_path_factory):
    status, r = R.run_host(exe, cases, tmp_path_factory.mktemp("ec_roots_cases"))
    print({k: v for k, v in r.items() if k != "groups"})
    for g, grp in enumerate(r["groups"]):
        if grp["pairs"]["compared"]:
            print(g, grp)
    return status, r


def test_inputs_are_the_ones_described(cases):
    assert len({c["glyph"] for c in cases if c["group"] == E.GROUP_GLYPHS}) == 40
    assert len([c for c in cases if c["group"] == E.GROUP_BENCH]) == 16 and all((c["w"], c["h"]) == (64, 64) for c in cases if c["group"] == E.GROUP_BENCH)
    crafted = [c for c in cases if "cells" in c]
    assert {(c["w"], c["h"]) for c in crafted} == set(R.CRAFTED_SIZES)
    for size in R.CRAFTED_SIZES:
        names = {n for c in crafted if (c["w"], c["h"]) == size for n in c["cells"]}
        assert names >= set(R.NAMED_CELLS) | {"non_finite", "random"}, size
    n = W.census([c["field"] for c in cases if c["group"] == R.GROUP_CRAFTED])
    assert all(n[k] >= 1 for k in W.KINDS), n


def test_same_verdicts_and_candidates_as_the_form_before(report, cases):
    status, r = report
    assert r["cases"] == len(cases)
    assert r["bad_verdict"] == 0 and r["bad_sink_list"] == 0 and r["bad_sink_direction"] == 0, r["bad_by_config"]
    assert r["bad_dense_verdict"] == 0 and r["bad_dense_sink_list"] == 0, r["bad_by_config"]
    assert status == 0
    assert len(r["bad_by_config"]) == 8 and {(d, o, p) for d, o, p, _ in r["bad_by_config"]} >= {(1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 2, 1)}
    assert r["comparisons"] > 1000000 and r["sink_calls"] > 1000


def test_not_vacuous(report):
    """At least 100 QUEUED items (what stage 1 hands to stage 2) of each kind, counted from the form before and the root predicates; the crafted cells
    reach every branch the rewrite touches; and a round of the dense form's emulation spills into a second chunk."""
    _, r = report
    total = {k: sum(g["items"][k] for g in r["groups"]) for k in r["groups"][0]["items"]}
    print(total)
    for k in R.BARS:
        assert total[k] >= 100, (k, total)
    crafted = r["groups"][R.GROUP_CRAFTED]["pairs"]
    for k in R.COVERED:
        assert crafted[k] >= 1, (k, crafted)
    assert sum(g["rounds"]["rounds_over_64_units"] for g in r["groups"]) >= 1
    assert max(r["case_max_units_per_round"]) > 64


def test_bench_sample_counts_are_consistent(report):
    """The round emulation on the bench sample: the lanes that reach the loop are those with one or two roots in range, and the passes of the new order
    are never more than the loop bodies of the old one."""
    _, r = report
    rd = r["groups"][E.GROUP_BENCH]["rounds"]
    assert rd["tiles"] == 16*64 and rd["rounds"] >= rd["tiles"]*.9
    assert rd["lanes_reaching_loop"] == rd["only_t0"]+rd["only_t1"]+rd["both_roots"]
    assert rd["after_passes"][0] == rd["rounds_reaching_loop"] and sum(rd["after_passes"]) <= sum(rd["before_body"])
    assert rd["after_rounds_first_extremum"]+rd["after_rounds_second_extremum"] <= sum(rd["before_extremum_blocks"])


def test_sanitized_build_of_the_host_program(cases, tmp_path_factory):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer (host code only), over the crafted fields and a fifth of the others. Skipped
    only where an EMPTY program cannot be built with those flags; any failure of the real build or run fails the test."""
    import subprocess
    import os
    tmp = tmp_path_factory.mktemp("ec_roots_host_san")
    src, probe = os.path.join(str(tmp), "probe.cpp"), os.path.join(str(tmp), "probe")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    b = subprocess.run(["g++", "-fsanitize=address,undefined", "-o", probe, src], capture_output=True)
    if b.returncode != 0 or subprocess.run([probe], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    san = R.build_host(tmp, sanitize=True)
    picked = [c for c in cases if c["group"] == R.GROUP_CRAFTED]+[c for c in cases if c["group"] not in (R.GROUP_CRAFTED, E.GROUP_BENCH)][::5]
    status, r = R.run_host(san, picked, tmp)
    assert status == 0 and r["cases"] == len(picked)
