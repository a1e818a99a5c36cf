"""msdf_prepplan.hpp -- which device buffers the raw-outline preparation touches, how large each is, how they are carved out of a slot, what every slot of a
streamed call must hold and which buffer feeds which field of PrepBuffers -- compiled with the host compiler (tests/hostemu). Every expected value is
restated here (numpy / plain Python), the slot sizes msdf_capi.hip computed inline before the plan existed included. The central check: a chunk carved
with its exact counts never ends beyond the slot that was sized from bounds; tests/prep_plan_host repeats it against real memory under the address and
undefined-behaviour sanitizers. No GPU."""
import ctypes as C
import itertools
import os
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from emu import Emu
from test_ec_lazy_host import _sanitizers_link

HOST_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "prep_plan_host", "prep_plan_host.cpp")

WAVE_MAX_EDGES = 2048                                                         # k_prep_colour_wave's large LDS tier
ORIENT_LDS_HITS = 1024                                                        # k_prep_orient's LDS tier
EDGE_REC = 384                                                                # sizeof(EdgeRec)
LIMIT32 = 0x7fffffff//8

Cfg = namedtuple("Cfg", "prepare coloring seeds raw_colors orient hits_big long_contour bounds records")
Counts = namedtuple("Counts", "n nC nE nE1 nE2")

UPLOADED = ["gco", "co", "raw_points", "raw_types", "raw_colors", "co1", "seeds"]
DEVICE_ONLY = ["cusp", "count", "co2", "norm_points", "norm_types", "norm_colors", "fin_points", "fin_types", "fin_colors", "big_mask", "big_spline",
               "big_edge_length", "big_corner_length", "big_corner_index", "big_minor", "votes", "hit_x", "hit_tag", "bounds", "recs", "windings"]
REGIONS = UPLOADED+DEVICE_ONLY

# region: (present under the configuration, bytes from the counts). e / e1 / e2: raw / normalized / coloured edges, one at least; ef: the final edges.
# Present iff a kernel of the queued sequence reads or writes it: k_prep_orient (raw, gco, co, votes, hits), k_prep_normalize_* (raw, co, co1, norm, cusp),
# k_prep_winding (norm), k_prep_count / k_prep_offsets (norm, co1, count, co2), k_prep_colour_wave (norm, co1, co2, seeds, fin, big), k_frame (norm, bounds),
# k_prep_records (the final arrays, recs, windings).
colouring = lambda c: c.prepare and c.coloring != 0
big = lambda c: colouring(c) and c.long_contour
big_ink = lambda c: big(c) and c.coloring == 2
hits = lambda c: c.prepare and c.orient and c.hits_big
TABLE = {
    "gco": (lambda c: True, lambda k: 4*(k.n+1)),
    "co": (lambda c: True, lambda k: 4*(k.nC+1)),
    "raw_points": (lambda c: True, lambda k: 64*k.e),
    "raw_types": (lambda c: True, lambda k: k.e),
    "raw_colors": (lambda c: c.raw_colors, lambda k: k.e),
    "co1": (lambda c: c.prepare, lambda k: 4*(k.nC+1)),
    "seeds": (lambda c: colouring(c) and c.seeds, lambda k: 8*k.n),
    "cusp": (lambda c: c.prepare, lambda k: 4*(k.nC+1)),
    "count": (colouring, lambda k: 4*(k.nC+1)),
    "co2": (colouring, lambda k: 4*(k.nC+1)),
    "norm_points": (lambda c: c.prepare, lambda k: 64*k.e1),
    "norm_types": (lambda c: c.prepare, lambda k: k.e1),
    "norm_colors": (lambda c: c.prepare, lambda k: k.e1),
    "fin_points": (colouring, lambda k: 64*k.e2),
    "fin_types": (colouring, lambda k: k.e2),
    "fin_colors": (colouring, lambda k: k.e2),
    "big_mask": (big, lambda k: 8*(k.e1//64+k.nC+2)),
    "big_spline": (big, lambda k: k.e1),
    "big_edge_length": (big_ink, lambda k: 8*k.e1),
    "big_corner_length": (big_ink, lambda k: 8*k.e1),
    "big_corner_index": (big_ink, lambda k: 4*k.e1),
    "big_minor": (big_ink, lambda k: k.e1),
    "votes": (lambda c: c.prepare and c.orient, lambda k: 4*(k.nC+1)),
    "hit_x": (hits, lambda k: 8*3*k.e),
    "hit_tag": (hits, lambda k: 4*3*k.e),
    "bounds": (lambda c: c.prepare and c.bounds, lambda k: 32*max(k.n, 1)),
    "recs": (lambda c: c.records, lambda k: EDGE_REC*k.ef),
    "windings": (lambda c: c.records, lambda k: max(k.nC, 1)),
}
assert sorted(TABLE) == sorted(REGIONS)


def model_sizes(cfg, counts):
    K = namedtuple("K", "n nC e e1 e2 ef")
    e, e1, e2 = max(counts.nE, 1), max(counts.nE1, 1), max(counts.nE2, 1)
    k = K(counts.n, counts.nC, e, e1, e2, e if not cfg.prepare else e2 if cfg.coloring else e1)
    return {r: (TABLE[r][1](k) if TABLE[r][0](cfg) else 0) for r in REGIONS}


def up256(x):
    return (x+255)//256*256


@pytest.fixture(scope="module")
def emu():
    e = Emu()
    uploaded = C.c_int(0)
    assert e.lib.emu_prep_regions(C.byref(uploaded)) == len(REGIONS) and uploaded.value == len(UPLOADED)
    return e


def carve(emu, cfg, counts):
    off, size, out = (C.c_longlong*len(REGIONS))(), (C.c_longlong*len(REGIONS))(), (C.c_longlong*3)()
    emu.lib.emu_prep_carve((C.c_int*9)(*[int(v) for v in cfg]), (C.c_longlong*5)(*counts), off, size, out)
    return dict(zip(REGIONS, off)), dict(zip(REGIONS, size)), {"upload": out[0], "device": out[1], "pinned": out[2]}


def plan_stream(emu, contours, edges, lengths, cfg):
    contours, edges, lengths = (np.ascontiguousarray(a, np.int32) for a in (contours, edges, lengths))
    chunks, out = np.zeros((len(lengths), 6), np.int64), (C.c_longlong*3)()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    n = emu.lib.emu_plan_stream_prep(ip(contours), ip(edges), ip(lengths), len(lengths), (C.c_int*9)(*[int(v) for v in cfg]),
                                     chunks.ctypes.data_as(C.POINTER(C.c_longlong)), out)
    return chunks[:n], {"pinned": out[0], "device": out[1], "refused": out[2]}


def prep_offsets(emu, co, normalize):
    co = np.ascontiguousarray(co, np.int32)
    co1, bound2, longest = np.full(len(co), -1, np.int32), C.c_longlong(-1), C.c_int(-1)
    emu.lib.emu_prep_offsets(co.ctypes.data_as(C.POINTER(C.c_int32)), len(co)-1, int(normalize), co1.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(bound2), C.byref(longest))
    return co1, bound2.value, longest.value


def model_offsets(sizes, normalize):
    """Shape::normalize splits a single-edge contour in thirds; a colouring splits a contour of fewer than three edges into three parts per edge at most."""
    sizes = np.asarray(sizes, np.int64)
    n1 = np.where(sizes == 1, 3, sizes) if normalize else sizes
    return np.concatenate([[0], np.cumsum(n1)]), int(np.where(n1 < 3, 3*n1, n1).sum()), int(n1.max(initial=0))


# ---------------------------------------------------------------------------------------------------------------- prepOffsets, orientHitsBig

@pytest.mark.parametrize("normalize", [False, True])
def test_prep_offsets_against_a_numpy_model(emu, normalize):
    rng = np.random.default_rng(20263)
    lists = [[], [0], [1], [2], [3], [0, 1, 2, 3, 2100], [1]*7, [2]*7, [2049, 0, 1, 2048]]
    lists += [rng.choice([0, 1, 2, 3, 4, 17, 300, 2500], int(rng.integers(1, 40))).tolist() for _ in range(200)]
    for sizes in lists:
        co = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        want_co1, want_bound2, want_longest = model_offsets(sizes, normalize)
        co1, bound2, longest = prep_offsets(emu, co, normalize)
        assert co1.tolist() == want_co1.tolist(), sizes
        assert (bound2, longest) == (want_bound2, want_longest), sizes


def test_orient_hits_beyond_the_lds_tier(emu):
    for raw, want in ((0, 0), (341, 0), (342, 1), (2100, 1), (2**31-1, 1)):
        assert 3*raw > ORIENT_LDS_HITS if want else 3*raw <= ORIENT_LDS_HITS
        assert emu.lib.emu_prep_orient_hits_big(C.c_longlong(raw)) == want, raw


# ---------------------------------------------------------------------------------------------------------------- region table and carve

ALL_CONFIGS = [Cfg(True, *flags) for flags in itertools.product((0, 1, 2), *[(False, True)]*7)]+[Cfg(False, 0, s, True, False, False, False, False, True) for s in (False, True)]
SOME_COUNTS = [Counts(0, 0, 0, 0, 0), Counts(1, 1, 1, 3, 9), Counts(5, 9, 40, 44, 52), Counts(64, 900, 3600, 3600, 3600), Counts(3, 3, 2102, 2104, 2110),
               Counts(255, 256, 257, 258, 259)]


def test_region_presence_and_sizes_for_every_configuration(emu):
    assert len(ALL_CONFIGS) == 3*2**7+2
    for cfg in ALL_CONFIGS:
        for counts in SOME_COUNTS:
            off, size, total = carve(emu, cfg, counts)
            assert size == model_sizes(cfg, counts), (cfg, counts)


def test_carve_is_aligned_ascending_disjoint_and_totalled(emu):
    for cfg in ALL_CONFIGS:
        for counts in SOME_COUNTS:
            off, size, total = carve(emu, cfg, counts)
            present = [r for r in REGIONS if size[r]]
            assert all(off[r] % 256 == 0 for r in present), (cfg, counts)
            for a, b in zip(present, present[1:]):                            # in table order, none reaching into the next
                assert off[a]+size[a] <= off[b], (cfg, counts, a, b)
            assert off[present[0]] == 0
            assert total["device"] == off[present[-1]]+size[present[-1]], (cfg, counts)
            uploaded = [r for r in present if r in UPLOADED]
            assert total["upload"] == up256(off[uploaded[-1]]+size[uploaded[-1]]), (cfg, counts)
            assert total["upload"] % 256 == 0 and all(off[r] >= total["upload"] for r in present if r in DEVICE_ONLY), (cfg, counts)
            # pinned staging: the uploaded part, and behind it the coloured offsets coming back
            assert total["pinned"] == total["upload"]+(4*(counts.nC+1) if cfg.prepare and cfg.coloring else 0), (cfg, counts)
            assert total["device"] <= sum(up256(s) for s in size.values())    # nothing is reserved twice


# ---------------------------------------------------------------------------------------------------------------- binder

FIELDS = ["gco", "co", "co1", "raw_points", "raw_types", "raw_colors", "norm_points", "norm_types", "norm_colors", "fin_points", "fin_types", "fin_colors", "cusp", "count",
          "co2", "seeds", "big_mask", "big_spline", "big_edge_length", "big_corner_length", "big_corner_index", "big_minor", "votes", "hit_x", "hit_tag"]   # PrepBuffers, in order


def test_binder_points_every_field_at_its_region(emu):
    base = 0x7f0000000000
    for cfg in ALL_CONFIGS:
        counts = Counts(5, 9, 40, 44, 52)
        off, size, total = carve(emu, cfg, counts)
        fields = (C.c_ulonglong*len(FIELDS))()
        emu.lib.emu_bind_prep(C.c_ulonglong(base), (C.c_int*9)(*[int(v) for v in cfg]), (C.c_longlong*5)(*counts), fields)
        got = dict(zip(FIELDS, fields))
        for f in FIELDS:
            region = f.replace("fin_", "norm_") if f.startswith("fin_") and not size["fin_points"] else f   # without a colouring the final edges are the normalized ones
            assert got[f] == (base+off[region] if size[region] else 0), (cfg, f)
        assert len({got[f] for f in FIELDS if size[f]}) == len([f for f in FIELDS if size[f]]), cfg     # distinct regions, distinct pointers


# ---------------------------------------------------------------------------------------------------------------- the streamed call's sizing

def parent_needs(contours, edges, lengths, prep, coloring, seeds, orient, frame):
    """What StreamFeeder::begin requested for a slot's pinnedIn / devIn (before the growth slack) when it sized the slots inline."""
    def layout(n, nC, nE):
        e = max(nE, 1)
        parts = [4*(n+1), 4*(nC+1), 64*e, e, e]+([4*(nC+1)] if prep else [])+([8*n] if prep and seeds else [])
        return sum(up256(p) for p in parts)

    def prep_layout(at, n, nC, nE, nE1, nE2, long_contour, hits_big):
        e, e1, e2 = max(nE, 1), max(nE1, 1), max(nE2, 1)
        parts = [4*(nC+1)]*3+[64*e1, e1, e1]
        if coloring:
            parts += [64*e2, e2, e2]
            if long_contour:
                parts += [8*(e1//64+nC+2), e1]+([8*e1, 8*e1, 4*e1, e1] if coloring == 2 else [])
        if orient:
            parts += [4*(nC+1)]+([24*e, 12*e] if hits_big else [])
        if frame:
            parts += [32*max(n, 1)]
        parts += [EDGE_REC*(e2 if coloring else e1), max(nC, 1)]
        return up256(at)+sum(up256(p) for p in parts)

    need_in = need_c = need_e = prep_pinned = prep_dev = 0
    g = 0
    for length in lengths:
        c, e = contours[g:g+length], edges[g:g+length]
        nC, nE = int(c.sum()), int(e.sum())
        bytes_ = layout(length, nC, nE)
        need_in, need_c, need_e = max(need_in, bytes_), max(need_c, nC), max(need_e, nE)
        if prep:
            may_have_long = bool((e.astype(np.int64)+2*c > WAVE_MAX_EDGES).any())
            hits_big = 3*int(e.max(initial=0)) > ORIENT_LDS_HITS
            prep_pinned = max(prep_pinned, up256(bytes_)+4*(nC+1))
            prep_dev = max(prep_dev, prep_layout(bytes_, length, nC, nE, nE+2*nC, nE+4*nC, may_have_long, hits_big))
        g += length
    if prep:
        return prep_pinned, prep_dev+256
    return need_in, need_in+up256(EDGE_REC*max(need_e, 1))+max(need_c, 1)+256


def glyph_list(rng, kind, n_glyphs):
    """Per glyph: the edge counts of its contours."""
    glyphs = []
    for _ in range(n_glyphs):
        n_contours = 0 if rng.random() < .15 else int(rng.integers(1, 8))
        if kind == "single":                                                  # every contour one edge: nE1 = nE + 2 nC exactly (with normalize)
            glyphs.append([1]*n_contours)
        elif kind == "pairs":                                                 # every contour two edges: the coloured bound is nE + 4 nC exactly
            glyphs.append([2]*n_contours)
        else:
            glyphs.append(rng.choice([0, 1, 2, 3, 5, 40], n_contours).tolist())
    return glyphs


TIER_GLYPHS = [[2046], [2047], [2045, 0], [2043, 1, 0], [2049], [2100, 3], [341], [342], [100, 241], [100, 242], [1]*1023, [1]*1025, []]


def schedules(rng, n_glyphs):
    yield [1]*n_glyphs
    yield [n_glyphs]
    for _ in range(3):
        lengths, left = [], n_glyphs
        while left:
            lengths.append(int(rng.integers(1, min(left, 9)+1)))
            left -= lengths[-1]
        yield lengths


STREAM_CONFIGS = [Cfg(True, coloring, seeds, True, orient, False, False, frame, True) for coloring in (0, 1, 2) for seeds in (False, True) for orient in (False, True)
                  for frame in (False, True)]+[Cfg(False, 0, False, True, False, False, False, False, True)]


def check_stream_call(emu, glyphs, lengths, cfg, normalize, rng):
    contours, edges = np.array([len(g) for g in glyphs], np.int32), np.array([sum(g) for g in glyphs], np.int32)
    chunks, need = plan_stream(emu, contours, edges, lengths, cfg)
    what = (cfg, lengths[:6], [g[:4] for g in glyphs[:4]])
    assert need["refused"] == -1 and len(chunks) == len(lengths), what
    parent_pinned, parent_dev = parent_needs(contours, edges, lengths, cfg.prepare, cfg.coloring, cfg.seeds, cfg.orient, cfg.bounds)
    assert need["pinned"] <= parent_pinned and need["device"]+256 <= parent_dev, (what, need, parent_pinned, parent_dev)
    g = 0
    for (start, length, nC, nE, may_have_long, hits_big), want_length in zip(chunks.tolist(), lengths):
        mine = glyphs[g:g+want_length]
        sizes = [n for glyph in mine for n in glyph]
        assert (start, length, nC, nE) == (g, want_length, len(sizes), sum(sizes)), what
        assert may_have_long == int(any(sum(glyph)+2*len(glyph) > WAVE_MAX_EDGES for glyph in mine)), what
        assert hits_big == int(3*max([sum(glyph) for glyph in mine], default=0) > ORIENT_LDS_HITS), what
        # the chunk as prepare() carves it: the real normalized count, the real longest contour and largest glyph, any coloured count up to the bound
        co1, bound2, longest = model_offsets(sizes, normalize)
        assert not (longest > WAVE_MAX_EDGES and not may_have_long), what
        for nE2 in {bound2, int(rng.integers(0, bound2+1))}:
            exact = cfg._replace(long_contour=longest > WAVE_MAX_EDGES, hits_big=bool(hits_big))
            counts = Counts(length, nC, nE, int(co1[-1]) if cfg.prepare else 0, nE2 if cfg.prepare else 0)
            off, size, total = carve(emu, exact, counts)
            assert total["device"] <= need["device"] and total["pinned"] <= need["pinned"], (what, g, counts, total, need)
            assert all(off[r]+size[r] <= need["device"] for r in REGIONS if size[r]), (what, g, counts)
            assert all(off[r]+size[r] <= need["pinned"] for r in UPLOADED if size[r]), (what, g, counts)
        g += want_length
    return chunks


def test_a_chunks_exact_carve_ends_inside_the_planned_slot(emu):
    rng = np.random.default_rng(20264)
    calls = 0
    for kind in ("mixed", "single", "pairs", "tiers"):
        for _ in range(6):
            n_glyphs = int(rng.integers(1, 30))
            glyphs = glyph_list(rng, kind, n_glyphs)
            if kind == "tiers":
                for at in rng.integers(0, n_glyphs, 4):
                    glyphs[at] = TIER_GLYPHS[int(rng.integers(0, len(TIER_GLYPHS)))]
            for lengths in schedules(rng, n_glyphs):
                for cfg in STREAM_CONFIGS:
                    check_stream_call(emu, glyphs, lengths, cfg, normalize=bool(rng.integers(0, 2)), rng=rng)
                    calls += 1
    assert calls >= 2000


def test_the_bounds_of_the_slot_sizing_are_attained(emu):
    """Single-edge contours reach nE + 2 nC normalized edges and two-edge contours nE + 4 nC coloured ones: there the exact carve of the largest chunk is the
    plan itself, so nothing smaller than these bounds would hold it."""
    rng = np.random.default_rng(20265)
    cfg = Cfg(True, 2, True, True, True, False, False, True, True)
    for sizes, normalize in (([1]*9, True), ([2]*9, True), ([2]*9, False)):
        glyphs = [sizes[:3], sizes[3:5], [], sizes[5:]]
        contours, edges = [len(g) for g in glyphs], [sum(g) for g in glyphs]
        co1, bound2, longest = model_offsets(sizes, normalize)
        if sizes[0] == 1:
            assert co1[-1] == sum(edges)+2*sum(contours)
        assert bound2 == sum(edges)+4*sum(contours) or sizes[0] == 1
        chunks, need = plan_stream(emu, contours, edges, [len(glyphs)], cfg)
        off, size, total = carve(emu, cfg, Counts(len(glyphs), len(sizes), sum(sizes), sum(edges)+2*sum(contours), sum(edges)+4*sum(contours)))
        assert (need["pinned"], need["device"]) == (total["pinned"], total["device"])
        check_stream_call(emu, glyphs, [len(glyphs)], cfg, normalize, rng)


@pytest.mark.parametrize("glyph, may_have_long, hits_big", [
    ([2046], 0, 1), ([2047], 1, 1), ([2044, 0], 0, 1), ([2045, 0], 1, 1),     # edges + 2 contours = 2 048 | 2 049
    ([341], 0, 0), ([342], 0, 1), ([100, 241], 0, 0), ([100, 242], 0, 1),     # 3 raw edges per hit slot: 1 023 | 1 026
    ([], 0, 0), ([0], 0, 0),
])
def test_tier_flags_of_a_chunk_switch_at_the_kernels_thresholds(emu, glyph, may_have_long, hits_big):
    cfg = Cfg(True, 2, False, True, True, False, False, False, True)
    chunks, need = plan_stream(emu, [0, len(glyph), 1], [0, sum(glyph), 3], [1, 1, 1], cfg)
    assert chunks[:, 4].tolist() == [0, may_have_long, 0] and chunks[:, 5].tolist() == [0, hits_big, 0]
    # the slot is sized for the chunk with the flags set, under a configuration that has the regions at all
    for flags_cfg in (cfg, cfg._replace(coloring=0), cfg._replace(orient=False)):
        n, nC, nE = 1, len(glyph), sum(glyph)
        long_regions, hit_regions = bool(may_have_long) and flags_cfg.coloring != 0, bool(hits_big) and flags_cfg.orient
        off, size, total = carve(emu, flags_cfg._replace(long_contour=bool(may_have_long), hits_big=bool(hits_big)), Counts(n, nC, nE, nE+2*nC, nE+4*nC))
        assert (size["big_mask"] > 0, size["big_minor"] > 0, size["hit_x"] > 0, size["hit_tag"] > 0) == (long_regions, long_regions, hit_regions, hit_regions)
        one, need_one = plan_stream(emu, [len(glyph)], [sum(glyph)], [1], flags_cfg)
        assert need_one["device"] == total["device"]


def test_chunks_beyond_32_bit_offsets_are_refused_at_the_same_counts(emu):
    prep, plain = Cfg(True, 1, False, True, False, False, False, False, True), Cfg(False, 0, False, True, False, False, False, False, True)
    refused = lambda contours, edges, lengths, cfg: plan_stream(emu, contours, edges, lengths, cfg)[1]["refused"]
    assert LIMIT32 == 268435455
    for cfg in (prep, plain):
        assert refused([1], [LIMIT32-4], [1], cfg) == -1
        assert refused([1], [LIMIT32+1], [1], cfg) == 0                       # edges
        assert refused([LIMIT32+1], [0], [1], cfg) == 0                       # contours
        assert refused([1, 1, 1], [5, LIMIT32+1, 5], [1, 1, 1], cfg) == 1     # the first chunk beyond, and the chunks up to it are described
        assert refused([1, 1, 1], [5, LIMIT32//2+1, LIMIT32//2+1], [1, 2], cfg) == 1    # a chunk's sum, not a glyph's count
        chunks, need = plan_stream(emu, [1, 1, 1], [5, LIMIT32+1, 5], [1, 1, 1], cfg)
        assert chunks[:, :4].tolist() == [[0, 1, 1, 5], [1, 1, 1, LIMIT32+1]]
    assert refused([LIMIT32], [0], [1], plain) == -1
    assert refused([LIMIT32], [0], [1], prep) == 0                            # raw outlines: the coloured bound nE + 4 nC counts
    assert refused([10], [LIMIT32-40], [1], prep) == -1
    assert refused([10], [LIMIT32-39], [1], prep) == 0
    assert refused([10], [LIMIT32-39], [1], plain) == -1
    # an accepted chunk of that size is planned in 64-bit sizes
    chunks, need = plan_stream(emu, [10], [LIMIT32-40], [1], prep)
    assert need["device"] > (64+64+EDGE_REC)*LIMIT32 and need["pinned"] > 64*(LIMIT32-40)


# ---------------------------------------------------------------------------------------------------------------- against real memory

def test_exact_carves_inside_arenas_of_the_planned_size_under_the_sanitizers(tmp_path):
    """tests/prep_plan_host: seeded random streamed calls in a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer (host code only):
    the slot as planned is malloc'ed, every chunk's present regions are memset over their full size. Skipped only where an EMPTY program cannot be built with
    those flags."""
    if not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    exe = os.path.join(str(tmp_path), "prep_plan_host_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, HOST_SRC],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.startswith("planned 600 calls, carved ") and int(r.stdout.split()[4]) >= 1500, r.stdout
