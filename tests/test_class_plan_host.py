"""planClasses (msdfgen_amd/csrc/msdf_classplan.hpp) -- the class list and ClassPlan that msdf_capi.hip's ensureBuckets uploads and the distance pass
launches from -- compiled with the host compiler (tests/hostemu) against a numpy restatement of its rules, on random glyphs and on the
boundaries of every class."""
import ctypes as C

import numpy as np
import pytest

from emu import Emu

LDS_LIMIT = 160*1024                                                          # a gfx950 CU's LDS, what msdfhip_init reads from the device


@pytest.fixture(scope="module")
def emu():
    return Emu()


def native_plan(emu, contours, edges, limit, small_max_edges, lds_limit):
    c, e = np.ascontiguousarray(contours, np.int32), np.ascontiguousarray(edges, np.int32)
    order = np.full(len(c), -1, np.int32)
    counts, share = np.zeros(8, np.int32), C.c_float()
    emu.lib.emu_class_plan(c.ctypes.data_as(C.POINTER(C.c_int)), e.ctypes.data_as(C.POINTER(C.c_int)), len(c), limit, small_max_edges, C.c_long(lds_limit),
                           order.ctypes.data_as(C.POINTER(C.c_int)), counts.ctypes.data_as(C.POINTER(C.c_int)), C.byref(share))
    return order, counts, share.value


def glyph_cost(c, e):
    """The cost model of the class plan: a + b*E + c*C + d*E*C per kernel class, never below the class's intercept."""
    coef = np.array([[0.25625, 0.01190, 0., 0.], [0.38398, 0.00846, -0.02755, 0.003446], [1.11611, 0.015776, -0.05039, 0.000681]])
    k = coef[np.where(c <= 1, 0, np.where((c <= 5) & (e <= 128), 1, 2))]
    return np.maximum(k[:, 0]+k[:, 1]*e+k[:, 2]*c+k[:, 3]*e.astype(np.float64)*c, k[:, 0])


def numpy_plan(c, e, limit, small_max_edges, lds_limit):
    c, e = np.asarray(c, np.int64), np.asarray(e, np.int64)
    huge = (e+4*c+2)*4 > lds_limit
    cls = np.where(huge, 3, np.where(c <= 1, 0, np.where((c <= limit) & (e <= small_max_edges), 1, 2)))
    weight = e*np.maximum(c, 1)
    lists = []
    for k in range(4):
        idx = np.flatnonzero(cls == k)
        lists.append(idx[np.argsort(-weight[idx], kind="stable")] if k < 3 else idx)   # heaviest first, ties in glyph order; the oversized ones in glyph order
    top = lambda a, idx: int(a[idx].max()) if len(idx) else 0
    counts = [len(lists[0]), len(lists[1]), len(lists[3]), top(e, lists[0]), top(c, lists[1]), top(e, lists[1]), top(c, lists[2]), top(e, lists[2])]
    cost = glyph_cost(c, e)
    share = cost[lists[2]].sum()/cost.sum() if cost.sum() > 0 else 1.
    return lists, counts, share


def glyph_set(limit, small_max_edges, lds_limit, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 3*limit+4, 200)
    e = np.where(rng.random(200) < .2, rng.integers(small_max_edges-3, small_max_edges+4, 200), rng.integers(0, 3*small_max_edges, 200))
    e = np.where(c == 0, 0, np.maximum(e, c))                                 # (a glyph without contours has no edges)
    over = lds_limit//4                                                       # e + 4 c + 2 > over: the survivor lists exceed the LDS limit
    edge = [(0, 0), (1, 0), (1, 1), (1, small_max_edges), (1, small_max_edges+1), (1, 3*small_max_edges),
            (2, small_max_edges), (2, small_max_edges+1), (limit, 7), (limit+1, 7), (limit, small_max_edges), (limit, small_max_edges+1),
            (limit+1, small_max_edges), (limit+1, small_max_edges+1),
            (3, over-4*3-2), (3, over-4*3-1), (1, over), (limit+9, over+50), (0, over),   # at the limit (kept), beyond it with 3 / 1 / many / no contours
            (2, 12), (3, 8), (1, 24), (4, 6), (2, 12), (6, 4), (1, 24), (24, 1), (0, 24), (1, 0), (0, 0)]   # ties in edges x max(contours, 1), over all classes
    c = np.concatenate([c, [p[0] for p in edge]]).astype(np.int32)
    e = np.concatenate([e, [p[1] for p in edge]]).astype(np.int32)
    perm = rng.permutation(len(c))
    return c[perm], e[perm]


@pytest.mark.parametrize("limit,small_max_edges,lds_limit", [(5, 128, LDS_LIMIT), (1, 128, LDS_LIMIT), (3, 96, LDS_LIMIT), (7, 160, 64*1024), (5, 128, 1200)])
def test_class_plan_matches_its_numpy_restatement(emu, limit, small_max_edges, lds_limit):
    c, e = glyph_set(limit, small_max_edges, lds_limit, 100+limit)
    order, counts, share = native_plan(emu, c, e, limit, small_max_edges, lds_limit)
    lists, want_counts, want_share = numpy_plan(c, e, limit, small_max_edges, lds_limit)
    assert (np.sort(order) == np.arange(len(c))).all(), "the class list is not a permutation of the glyphs"
    assert counts.tolist() == want_counts, (counts.tolist(), want_counts)
    assert all(len(l) >= 3 for k, l in enumerate(lists) if k != 1 or limit > 1), "the glyph set misses a class: %s" % [len(l) for l in lists]   # (limit 1: no LDS class)
    at = 0
    for k, name in enumerate(("one contour", "LDS", "global scratch", "oversized")):
        assert (order[at:at+len(lists[k])] == lists[k]).all(), name
        at += len(lists[k])
    assert share == pytest.approx(want_share, rel=1e-6)
    assert 0 < share < 1


def test_class_plan_of_no_glyphs_and_of_one_class(emu):
    order, counts, share = native_plan(emu, [], [], 5, 128, LDS_LIMIT)
    assert counts.tolist() == [0]*8 and share == 1.
    order, counts, share = native_plan(emu, [1, 0, 1], [9, 0, 30], 5, 128, LDS_LIMIT)           # nothing in the global-scratch class
    assert order.tolist() == [2, 0, 1] and counts.tolist() == [3, 0, 0, 30, 0, 0, 0, 0] and share == 0.
    order, counts, share = native_plan(emu, [9, 7], [40, 300], 5, 128, LDS_LIMIT)               # nothing but that class
    assert order.tolist() == [1, 0] and counts.tolist() == [0, 0, 0, 0, 0, 0, 9, 300] and share == 1.
