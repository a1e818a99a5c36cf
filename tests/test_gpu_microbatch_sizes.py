"""Concurrent single-shape calls of DIFFERENT bitmap sizes in one micro-batch group (msdf_groupplan.hpp, runGroup's mixed path, k_boxes_to_slots): every
front-door entry point, each call into a caller bitmap with a padded or a negative row stride, against the oracle per call at that call's own size -- bits, as
tests/test_gpu_sized.py compares them. Glyphs, boxes and framing are that file's: its synthesizers, its BOXES cycle, autoframe per box.

Grouping is forced, not hoped for: one leader slot, a hold (msdfhip_microbatch_hold) under which every call of a case queues up in a known arrival order,
then one release. The hold is bounded, every thread is joined with a timeout: a failure cannot park the suite."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

import msdfgen_amd as M
import fuzzlib
from msdfgen_amd import lib as L
from msdfgen_amd.shape import autoframe
from test_gpu_sized import BOXES, SENTINEL, glyphs

pytestmark = pytest.mark.gpu
T = 2*len(BOXES)                                                            # 22 calls: two turns of BOXES
SLOT = 24*17
KNOB = "MSDFHIP_MICROBATCH_MAX_PAD"
GEN, EC, SIGN, RASTER, LEGACY = "generate", "error_correction", "sign_correction", "rasterize", "legacy"


def set_max_pad(value):
    os.environ[KNOB] = str(value)
    L.load().msdfhip_reload_tuning()


@pytest.fixture(scope="module", autouse=True)
def _one_leader():
    M.init(0)
    assert M.device_info()["arch"].startswith("gfx950")
    before = os.environ.get(KNOB)
    M.set_microbatch(256, 1)
    yield
    M.set_microbatch(256, 4)
    if before is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = before
    L.load().msdfhip_reload_tuning()


class Call:
    """One front-door call into a bitmap of its own: the box sits one texel inside a sentinel-filled buffer whose rows are two texels longer than the box's
    (a padded row stride); every second call addresses its rows bottom-up (a negative row stride)."""

    def __init__(self, k, op, shape, w, h, xf, n, mode=0, cfg=None, y_down=False, field=None, want=None, want_stencil=None, zero=.5, rule=0):
        self.op, self.shape, self.w, self.h, self.n, self.mode, self.want, self.want_stencil = op, shape, w, h, n, mode, want, want_stencil
        self.negative = k % 2 == 1
        self.stride = (w+2)*n
        self.buf = np.full((h+2, self.stride), SENTINEL, np.uint32).view(np.float32)
        self.zero, self.rule = zero, rule
        # xf as shape.autoframe() gives it (projection, then the range); the C ABI takes the projection and the distance mapping (LEGACY: given as such)
        xf = np.asarray(xf, np.float64).reshape(-1)
        self.xf = np.ascontiguousarray(M.SDFTransformation.from_xf(xf).xf6() if op in (GEN, EC) else xf[:6] if op == LEGACY else list(xf[:4])+[1, 0], np.float64)
        self.cfg = cfg
        self.flip = int(bool(shape.inverse_y) != bool(y_down))
        self.stencil = np.full(w*h+8, 77, np.uint8) if want_stencil is not None else None
        if field is not None:
            self.box()[...] = field
        self.co = np.ascontiguousarray(shape.contour_offsets, np.int32)
        self.pts = np.ascontiguousarray(shape.points, np.float64)
        self.types, self.colors = np.ascontiguousarray(shape.types, np.uint8), np.ascontiguousarray(shape.colors, np.uint8)
        self.rc, self.error = None, None

    def box(self):
        """The bitmap as the call sees it, (h, w, n): row 0 is the memory-last row under a negative stride."""
        v = self.buf[1:self.h+1, self.n:(self.w+1)*self.n].reshape(self.h, self.w, self.n)
        return v[::-1] if self.negative else v

    def run(self):
        try:
            lib = L.load()
            first = self.buf[self.h if self.negative else 1, self.n:]
            px = first.ctypes.data_as(L._fp)
            stride = -self.stride if self.negative else self.stride
            sargs = (L.ptr(self.co, L._ip), self.shape.n_contours, L.ptr(self.pts, L._dp), L.ptr(self.types, L._bp), L.ptr(self.colors, L._bp))
            st = L.ptr(self.stencil, L._bp) if self.stencil is not None else None
            xf = L.ptr(self.xf, L._dp)
            if self.op == GEN:
                self.rc = lib.msdfhip_generate(self.mode, px, self.w, self.h, stride, self.flip, *sargs, xf, C.byref(self.cfg), st)
            elif self.op == LEGACY:
                self.rc = lib.msdfhip_generate_legacy(self.mode, px, self.w, self.h, stride, self.flip, *sargs, xf, C.byref(self.cfg), st)
            elif self.op == EC:
                self.rc = lib.msdfhip_error_correction(self.n, px, self.w, self.h, stride, self.flip, *sargs, xf, C.byref(self.cfg), st)
            elif self.op == SIGN:
                self.rc = lib.msdfhip_distance_sign_correction(self.n, px, self.w, self.h, stride, self.flip, *sargs, xf, self.zero, self.rule)
            else:
                self.rc = lib.msdfhip_rasterize(px, self.w, self.h, stride, self.flip, *sargs, xf, self.rule)
            if self.rc != 0:
                self.error = lib.msdfhip_last_error()
        except Exception as e:  # noqa: BLE001
            self.error = repr(e)

    def differing(self):
        """(float values whose bits differ from the oracle's, stencil bytes that differ, sentinel texels that were written)."""
        assert self.rc == 0 and self.error is None, (self.op, self.w, self.h, self.rc, self.error)
        got, want = np.ascontiguousarray(self.box()), np.asarray(self.want, np.float32).reshape(self.h, self.w, self.n)
        bad = int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).sum())
        st = 0
        if self.stencil is not None:
            st = int((self.stencil[:self.w*self.h].reshape(self.h, self.w) != self.want_stencil).sum())+int((self.stencil[self.w*self.h:] != 77).sum())
        outside = np.ones(self.buf.shape, bool)
        outside[1:self.h+1, self.n:(self.w+1)*self.n] = False
        return bad, st, int((self.buf.view(np.uint32)[outside] != SENTINEL).sum())


def run_held(calls, hold_ms=20000):
    """Every call on a thread of its own, queued under a hold in the order of `calls` (a thread starts once its predecessor is queued), then one release."""
    threads = [threading.Thread(target=c.run) for c in calls]
    with M.microbatch_hold(hold_ms) as hold:
        deadline = time.monotonic()+15
        for k, t in enumerate(threads):
            t.start()
            while hold.queued() < k+1 and t.is_alive() and time.monotonic() < deadline:
                time.sleep(.0005)
        queued = hold.queued()
    for t in threads:
        t.join(30)
    assert not any(t.is_alive() for t in threads), "a call did not return"
    assert queued == len(calls), (queued, len(calls))


def check(calls, what):
    bad = st = outside = values = 0
    for c in calls:
        b, s, o = c.differing()
        bad, st, outside, values = bad+b, st+s, outside+o, values+c.w*c.h*c.n
    print({"case": what, "values_compared": values, "values_differing_bitwise": bad, "stencil_values_differing": st, "sentinels_written": outside})
    assert values > 0 and (bad, st, outside) == (0, 0, 0), what


def stats_of(fn):
    M.microbatch_stats(reset=True)
    fn()
    st = M.microbatch_stats()
    return {k: st[k] for k in ("calls", "batches", "largest", "mixed_batches", "mixed_calls", "padded_texels", "box_texels")}


def config(overlap=1, ec_mode=M.EC_EDGE_PRIORITY, ec_dist=M.CHECK_DISTANCE_AT_EDGE, y_down=False, sign=None):
    cfg = L.default_config(overlap_support=overlap, ec_mode=ec_mode, ec_distance_check=ec_dist, stencil_y_down=int(y_down))
    if sign is not None:
        cfg.sign_correction, cfg.fill_rule, cfg.sdf_zero_value = 1, sign, .5
    return cfg


_REF = {}


def generated(oracle, g, w, h, xf, mode, overlap, ec_mode, ec_dist, y_down, sign):
    """The oracle's bitmap and stencil of glyph g at w x h: computed once per configuration, never written to."""
    key = (g, w, h, mode, overlap, ec_mode, ec_dist, y_down, sign)
    if key not in _REF:
        s = glyphs()[0][g]
        sb = np.zeros((h, w), np.uint8)
        if sign is None:
            f = oracle.generate(s, mode, w, h, xf, overlap=bool(overlap), ec_mode=ec_mode, ec_dist=ec_dist, y_down=y_down, stencil=sb)
        else:                                                               # the -scanline flow: field -> sign pass -> correction
            f = oracle.generate(s, mode, w, h, xf, overlap=bool(overlap), ec_mode=0, y_down=y_down)
            f = oracle.sign_correction(s, f, xf, .5, sign, y_down=y_down)
            if mode >= 3 and ec_mode != 0:
                f = oracle.error_correction(s, f, xf, overlap=bool(overlap), ec_mode=ec_mode, ec_dist=ec_dist, y_down=y_down, stencil=sb)
        f.setflags(write=False), sb.setflags(write=False)
        _REF[key] = (f, sb)
    return _REF[key]


def generate_calls(oracle, mode, overlap=1, ec_mode=M.EC_EDGE_PRIORITY, ec_dist=M.CHECK_DISTANCE_AT_EDGE, y_down=False, sign=None, boxes=None):
    shapes, sizes, xfs = glyphs()
    calls = []
    for k in range(T if boxes is None else len(boxes)):
        w, h = (int(v) for v in (sizes[k] if boxes is None else boxes[k]))
        xf = xfs[k] if boxes is None else autoframe(shapes[k].bounds(), w, h, min(2., .5*min(w, h)))
        want, want_st = generated(oracle, k, w, h, xf, mode, overlap, ec_mode, ec_dist, y_down, sign)
        stencil = want_st if mode >= 3 and ec_mode != 0 else None
        calls.append(Call(k, GEN, shapes[k], w, h, xf, M.CHANNELS[mode], mode=mode, cfg=config(overlap, ec_mode, ec_dist, y_down, sign), y_down=y_down, want=want,
                          want_stencil=stencil))
    return calls


def test_the_inputs_are_the_ones_described():
    shapes, sizes, _ = glyphs()
    assert [tuple(b) for b in sizes[:T].tolist()] == list(BOXES)*2 and (int(sizes[:T, 0].max())*int(sizes[:T, 1].max())) == SLOT
    assert any(s.inverse_y for s in shapes[:T]) and not all(s.inverse_y for s in shapes[:T])
    assert sum(w*h for w, h in BOXES) == 1538


def test_msdf_calls_of_eleven_sizes_run_as_one_group(oracle):
    """Case 1: 22 generateMSDF calls, default config, with stencils -> ONE device batch with sizes. Without the feature the calls run as one batch per distinct
    size (11 batches, largest 2)."""
    set_max_pad(1000)
    calls = generate_calls(oracle, 3)
    st = stats_of(lambda: run_held(calls))
    print(st)
    check(calls, "msdf, default config")
    assert st == {"calls": T, "batches": 1, "largest": T, "mixed_batches": 1, "mixed_calls": T, "padded_texels": T*SLOT, "box_texels": 2*1538}


@pytest.mark.parametrize("what,kw", [("sdf", dict(mode=1)), ("psdf", dict(mode=2)), ("mtsdf", dict(mode=4)), ("simple combiner", dict(mode=3, overlap=0)),
                                     ("mtsdf, simple combiner, every texel checked", dict(mode=4, overlap=0, ec_mode=M.EC_INDISCRIMINATE, ec_dist=M.ALWAYS_CHECK_DISTANCE)),
                                     ("scanline pass, nonzero", dict(mode=3, sign=M.FILL_NONZERO)), ("scanline pass, odd", dict(mode=4, sign=M.FILL_ODD)),
                                     ("scanline pass, sdf, positive", dict(mode=1, sign=M.FILL_POSITIVE)), ("y down", dict(mode=3, y_down=True)),
                                     ("y down, mtsdf", dict(mode=4, y_down=True))])
def test_generate_calls_of_eleven_sizes_vs_oracle(oracle, what, kw):
    """Case 2, the generators: modes 1, 2 and 4, both combiners, the sign pass under fill rules, Y-down groups (`flip` varies per call with the shape's own
    orientation; the stencils keep the reference's upward rows)."""
    set_max_pad(1000)
    calls = generate_calls(oracle, **kw)
    assert len({c.flip for c in calls}) == 2
    st = stats_of(lambda: run_held(calls))
    check(calls, what)
    assert (st["calls"], st["batches"], st["largest"], st["mixed_batches"], st["padded_texels"], st["box_texels"]) == (T, 1, T, 1, T*SLOT, 2*1538), st


@pytest.mark.parametrize("mode", [3, 4])
def test_error_correction_calls_of_eleven_sizes_vs_oracle(oracle, mode):
    """Case 2, msdfhip_error_correction in place on uncorrected fields: the packed bitmaps reach their slots through k_boxes_to_slots."""
    set_max_pad(1000)
    shapes, sizes, xfs = glyphs()
    calls = []
    for k in range(T):
        w, h = int(sizes[k, 0]), int(sizes[k, 1])
        field, _ = generated(oracle, k, w, h, xfs[k], mode, 1, 0, 0, False, None)             # the correction disabled at generation
        sb = np.zeros((h, w), np.uint8)
        want = oracle.error_correction(shapes[k], field, xfs[k], stencil=sb)
        calls.append(Call(k, EC, shapes[k], w, h, xfs[k], M.CHANNELS[mode], cfg=config(), field=field, want=want, want_stencil=sb))
    st = stats_of(lambda: run_held(calls))
    check(calls, "error correction, %d channels" % M.CHANNELS[mode])
    assert (st["batches"], st["largest"], st["mixed_batches"]) == (1, T, 1), st


@pytest.mark.parametrize("mode,rule", [(1, M.FILL_NONZERO), (3, M.FILL_ODD), (4, M.FILL_NONZERO)])
def test_sign_correction_calls_of_eleven_sizes_vs_oracle(oracle, mode, rule):
    """Case 2, msdfhip_distance_sign_correction in place on INVERTED fields (every texel has to flip)."""
    set_max_pad(1000)
    shapes, sizes, xfs = glyphs()
    calls = []
    for k in range(T):
        w, h = int(sizes[k, 0]), int(sizes[k, 1])
        field = 1-generated(oracle, k, w, h, xfs[k], mode, 1, 0, 0, False, None)[0]
        want = oracle.sign_correction(shapes[k], field, xfs[k], .5, rule)
        calls.append(Call(k, SIGN, shapes[k], w, h, xfs[k], M.CHANNELS[mode], field=field, want=want, rule=rule))
    assert any((np.asarray(c.want) != np.asarray(c.box())).any() for c in calls)
    st = stats_of(lambda: run_held(calls))
    check(calls, "sign correction, %d channels" % M.CHANNELS[mode])
    assert (st["batches"], st["largest"], st["mixed_batches"]) == (1, T, 1), st


def test_rasterize_calls_of_eleven_sizes_vs_oracle(oracle):
    set_max_pad(1000)
    shapes, sizes, xfs = glyphs()
    calls = [Call(k, RASTER, shapes[k], int(sizes[k, 0]), int(sizes[k, 1]), xfs[k], 1, want=oracle.rasterize(shapes[k], int(sizes[k, 0]), int(sizes[k, 1]), xfs[k], M.FILL_NONZERO),
                  rule=M.FILL_NONZERO) for k in range(T)]
    st = stats_of(lambda: run_held(calls))
    check(calls, "rasterize")
    assert (st["batches"], st["largest"], st["mixed_batches"]) == (1, T, 1), st


def test_max_pad_zero_groups_by_size_and_gives_the_same_bytes(oracle):
    """Case 3: MSDFHIP_MICROBATCH_MAX_PAD=0 is the grouping by equal size: one batch per distinct size, none with sizes, the bytes of case 1."""
    set_max_pad(1000)
    mixed = generate_calls(oracle, 3)
    run_held(mixed)
    set_max_pad(0)
    calls = generate_calls(oracle, 3)
    st = stats_of(lambda: run_held(calls))
    check(calls, "msdf, MAX_PAD=0")
    assert (st["calls"], st["batches"], st["largest"], st["mixed_batches"], st["mixed_calls"]) == (T, len(BOXES), 2, 0, 0), st
    for a, b in zip(mixed, calls):
        assert np.ascontiguousarray(a.box()).tobytes() == np.ascontiguousarray(b.box()).tobytes() and (a.stencil == b.stencil).all()


def big_and_small(oracle, big_first):
    boxes = [(64, 64)]+[(8, 8)]*10 if big_first else [(8, 8)]*10+[(64, 64)]
    return generate_calls(oracle, 3, boxes=boxes)


@pytest.mark.parametrize("big_first", [False, True])
def test_padding_bound_keeps_large_and_small_calls_apart(oracle, big_first):
    """Case 4, MAX_PAD=2: one 64 x 64 call and ten 8 x 8 calls, under either arrival order: no group holds both kinds (largest <= 10, mixed_batches == 0), all
    results right. (The bound on every member keeps them apart when the large call leads: 4096 > 2*64; the bound on the whole group alone would admit
    that pair, 2*4096 <= 2*4160.)"""
    set_max_pad(2)
    calls = big_and_small(oracle, big_first)
    st = stats_of(lambda: run_held(calls))
    print(st)
    check(calls, "64x64 %s ten 8x8, MAX_PAD=2" % ("before" if big_first else "after"))
    assert st["calls"] == 11
    assert st["largest"] <= 10 and st["mixed_batches"] == 0, st


@pytest.mark.parametrize("big_first", [False, True])
def test_a_generous_padding_bound_takes_large_and_small_calls_together(oracle, big_first):
    """Case 4, MAX_PAD=1000: one group of 11."""
    set_max_pad(1000)
    calls = big_and_small(oracle, big_first)
    st = stats_of(lambda: run_held(calls))
    check(calls, "64x64 and ten 8x8, MAX_PAD=1000")
    assert st == {"calls": 11, "batches": 1, "largest": 11, "mixed_batches": 1, "mixed_calls": 11, "padded_texels": 11*4096, "box_texels": 4096+640}


def test_equal_sizes_take_the_launches_they_always_took(oracle):
    """Case 5: 16 calls of one size: no group with sizes, the bytes of lone calls, and the route counters of the same run with MAX_PAD=0."""
    boxes = [(16, 16)]*16
    lone = generate_calls(oracle, 3, boxes=boxes)
    for c in lone:
        c.run()
    check(lone, "lone 16x16 calls")
    runs = {}
    for pad in (5, 0):
        set_max_pad(pad)
        calls = generate_calls(oracle, 3, boxes=boxes)
        before = M.route_counts()
        st = stats_of(lambda: run_held(calls))
        runs[pad] = (fuzzlib._delta(M.route_counts(), before), st)
        check(calls, "16 equal calls, MAX_PAD=%d" % pad)
        assert (st["calls"], st["batches"], st["largest"], st["mixed_batches"], st["padded_texels"]) == (16, 1, 16, 0, 0), st
        for a, b in zip(lone, calls):
            assert np.ascontiguousarray(a.box()).tobytes() == np.ascontiguousarray(b.box()).tobytes() and (a.stencil == b.stencil).all()
    assert runs[5] == runs[0] and sum(runs[5][0].values()) > 0, runs


def test_legacy_calls_never_mix_sizes():
    """Case 6: legacy generator calls of three sizes under one hold: three batches, none with sizes, the recorded reference's bytes (tests/golden/legacy.npz)."""
    import legacycases as LC
    set_max_pad(1000)
    batch, recs, _ = LC.golden()
    picked = []
    for size in ((7, 5), (8, 8), (9, 17)):
        same = [r for r in recs if (r.mode, r.ec, r.y_down, r.sign, r.stencil is None, (r.w, r.h)) == (3, 2, False, False, True, size)]
        assert same, size
        picked += [same[0], same[-1]]
    calls = [Call(k, LEGACY, batch.shape(r.shape), r.w, r.h, LC.xf6(r.xf), 3, mode=3, cfg=L.default_config(ec_mode=r.ec, stencil_y_down=0), want=r.out)
             for k, r in enumerate(picked)]
    st = stats_of(lambda: run_held(calls))
    check(calls, "legacy msdf, three sizes")
    assert (st["calls"], st["batches"], st["largest"], st["mixed_batches"]) == (6, 3, 2, 0), st


def test_a_hold_nobody_releases_ends_by_itself(oracle):
    """Case 7: microbatch_hold(200) never released: a lone call waits the hold out on the host and returns the right bytes."""
    set_max_pad(1000)
    c = generate_calls(oracle, 3)[7]
    lib = L.load()
    assert lib.msdfhip_microbatch_hold(200) == 0
    t0 = time.monotonic()
    t = threading.Thread(target=c.run)
    t.start()
    t.join(30)
    waited = time.monotonic()-t0
    assert not t.is_alive()
    assert lib.msdfhip_microbatch_hold(0) == 0
    check([c], "a call under an expiring hold")
    assert .1 < waited < 10, waited
