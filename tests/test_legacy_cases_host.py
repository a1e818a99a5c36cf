"""The legacy route on every framing family (xformcases), every outline family (geomcases) and seeded random outlines, without a GPU: the host build of
msdf_legacy.hpp (tests/legacy_host), the reference of a legacy call that the GPU tests compare with (legacycases.reference_call) and the device
correction as the legacy entry points invoke it (tests/hostemu), each against the compiled reference called now. The tests that take `ref` skip where
it is not built; what has to hold without it is checked against recorded data. Every comparison is bitwise, a NaN equal to a NaN only."""
import numpy as np
import pytest

import geomcases as GC
import legacycases as LC
import xformcases as XC

CORRECTED = ((3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (4, 3))       # (mode, ErrorCorrectionConfig::Mode)
THE_CASE = "degenerate_edges/cubic_p2_on_p3"                        # at 12x12: the stencil byte that tells the shape's row order from the bitmap's


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return LC.build_host(tmp_path_factory.mktemp("legacy_host"))


@pytest.fixture(scope="module")
def emu():
    from emu import Emu
    return Emu()


@pytest.fixture(scope="module")
def sets():
    """(framing cases, outline cases, random outlines): computed once, never changed."""
    return XC.cases(seeds=(0, 1)), GC.cases(), LC.fuzz_cases()


@pytest.fixture(scope="module")
def rl(ref):
    return LC.RefLegacy(ref)


def test_case_sets_are_what_the_tests_below_assume(sets):
    framing, outline, fuzz = sets
    assert len(framing) == 84 and len(outline) == 56 and len(fuzz) == 60
    assert {c.name.split("/")[0] for c in framing} == set(XC.FAMILIES) and {c.name.split("/")[0] for c in outline} == set(GC.FAMILIES)
    for c in framing:
        XC.check_premise(c)
    assert any(c.xf[0] < 0 for c in framing) and any(c.xf[1] < 0 for c in framing)
    assert {(bool(c.shape.inverse_y), c.y_down) for c in framing} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(bool(c.shape.inverse_y), c.y_down) for c in fuzz} == {(False, False), (False, True), (True, False), (True, True)}
    assert min(c.w for c in fuzz) < 8 and min(c.h for c in fuzz) < 8 and max(c.w for c in fuzz) > 32
    # bit_exact takes out the cases of one base name, and nothing else
    kept = GC.bit_exact(outline)
    gone = [c for c in outline if c not in kept]
    assert GC.SIGN_NOISE == ("degenerate_edges/quad_fold_back",)
    assert gone and {GC.base_name(c) for c in gone} == set(GC.SIGN_NOISE)
    assert len(kept) == len(outline)-sum(GC.base_name(c) in GC.SIGN_NOISE for c in outline)
    assert GC.bit_exact(framing) == framing and GC.bit_exact(fuzz) == fuzz
    the = [c for c in kept if GC.base_name(c) == THE_CASE]
    assert the and all((c.w, c.h) == (12, 12) and not c.shape.inverse_y for c in the)


def test_raw_fields_equal_the_reference(rl, host, sets):
    """legacyTexel compiled for the host against generate*_legacy with the correction off: all three sets (the sign-noise case included: libm on both
    sides), all four modes."""
    values = 0
    for cs in sets:
        for c in cs:
            for mode in (1, 2, 3, 4):
                want = rl.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
                got = LC.host_generate(host, c.shape, mode, c.w, c.h, c.xf, c.y_down)
                assert np.isfinite(got).all() == np.isfinite(want).all()
                assert LC.differing(got, want) == 0, (c.name, mode)
                values += got.size
    print("raw legacy fields: %d values, 0 differ" % values)
    assert values > 900000


def test_helper_equals_the_reference_without_the_sign_pass(rl, host, oracle, sets):
    """reference_call against generateMSDF_legacy / generateMTSDF_legacy under every correction mode: pixels and stencils."""
    framing, outline, fuzz = sets
    values = texels = 0
    for c in framing+GC.bit_exact(outline)+fuzz:
        for mode, ec in CORRECTED:
            st = np.zeros((c.h, c.w), np.uint8)
            want = rl.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=ec, y_down=c.y_down, stencil=st)
            got, gs = LC.reference_call(host, oracle, c.shape, mode, c.w, c.h, c.xf, ec_mode=ec, y_down=c.y_down)
            assert LC.differing(got, want) == 0, (c.name, mode, ec)
            assert np.array_equal(gs, st), (c.name, mode, ec, np.argwhere(gs != st).tolist()[:4])
            values, texels = values+got.size, texels+st.size
    print("helper, no sign pass: %d values and %d stencil bytes, 0 differ" % (values, texels))


def test_helper_equals_the_reference_with_the_sign_pass(ref, rl, host, oracle, sets):
    """reference_call(sign=...) against the CLI's order run on the compiled reference: legacy field -> distanceSignCorrection -> msdfErrorCorrection on
    the bitmap as it lies. Every third case of the framing and the outline lists, all fill rules, two zero levels."""
    framing, outline, _ = sets
    values = 0
    for c in (framing+outline)[::3]:
        for mode, ec in ((1, 0), (3, 0), (3, 2), (4, 1)):
            raw = rl.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=0, y_down=c.y_down)
            for rule in range(4):
                for zero in (.5, .3):
                    want = ref.sign_correction(c.shape, raw, c.xf, zero=zero, fill_rule=rule, y_down=c.y_down)
                    st = np.zeros((c.h, c.w), np.uint8)
                    if ec:
                        want = ref.error_correction(c.shape, want, c.xf, overlap=False, ec_mode=ec, ec_dist=0, y_down=c.y_down, stencil=st)
                    got, gs = LC.reference_call(host, oracle, c.shape, mode, c.w, c.h, c.xf, ec_mode=ec, y_down=c.y_down, sign=LC.SignPass(rule, zero))
                    assert LC.differing(got, want) == 0, (c.name, mode, ec, rule, zero)
                    if ec:
                        assert np.array_equal(gs, st), (c.name, mode, ec, rule, zero)
                    values += got.size
    print("helper, sign pass: %d values, 0 differ" % values)


def test_helper_reproduces_the_recorded_cli_flow(host, oracle):
    """The two default_flow records of tests/golden/legacy.npz (the reference CLI's own output): no compiled reference needed."""
    batch, recs, _ = LC.golden()
    flows = [r for r in recs if r.sign]
    assert [r.mode for r in flows] == [3, 4]
    for r in flows:
        got, _ = LC.reference_call(host, oracle, batch.shape(r.shape), r.mode, r.w, r.h, r.xf, ec_mode=r.ec, y_down=r.y_down, sign=LC.SignPass(r.fill, r.zero))
        assert LC.differing(got, r.out) == 0, r.name
    for r in (r for r in recs if not r.sign):                                  # and every other record, stencils included
        got, gs = LC.reference_call(host, oracle, batch.shape(r.shape), r.mode, r.w, r.h, r.xf, ec_mode=r.ec, y_down=r.y_down)
        assert LC.differing(got, r.out) == 0, r.name
        if r.stencil is not None:
            assert np.array_equal(gs, r.stencil), r.name


def test_device_correction_as_the_legacy_entry_points_invoke_it(rl, host, emu, sets):
    """The device's correction compiled for the host (tests/hostemu), called as runGenerateLegacy calls it without the sign pass -- no overlap support, no
    distance check, protectEdges' pairs along the shape's rows -- on the host build's raw field, against generateMSDF_legacy / generateMTSDF_legacy with
    a stencil: every bit-exact case under BOTH bitmap orientations. With the pairs along the bitmap's rows one stencil byte of cubic_p2_on_p3 at 12x12
    (upward shape, Y-down bitmap, EDGE_PRIORITY) departs."""
    framing, outline, fuzz = sets
    seen_the_case = False
    values = texels = 0
    for c in framing+GC.bit_exact(outline)+fuzz:
        for y_down in (False, True):
            for mode, ec in CORRECTED:
                st = np.zeros((c.h, c.w), np.uint8)
                want = rl.generate(c.shape, mode, c.w, c.h, c.xf, ec_mode=ec, y_down=y_down, stencil=st)
                raw = LC.host_generate(host, c.shape, mode, c.w, c.h, c.xf, y_down)
                se = np.zeros((c.h, c.w), np.uint8)
                got = emu.generate(c.shape, mode, c.w, c.h, c.xf, overlap=False, ec_mode=ec, ec_dist=0, y_down=y_down, correct_only=raw, stencil=se, shape_rows=True)
                se = se[::-1] if y_down else se                                # stencilIndex: the stencil's rows go upward whatever the bitmap's
                assert LC.differing(got, want) == 0, (c.name, y_down, mode, ec)
                assert np.array_equal(se, st), (c.name, y_down, mode, ec, np.argwhere(se != st).tolist()[:4])
                values, texels = values+got.size, texels+st.size
                if GC.base_name(c) == THE_CASE and (c.w, c.h) == (12, 12) and not c.shape.inverse_y and y_down and (mode, ec) == (3, 2):
                    seen_the_case = True
                    plain = np.zeros((c.h, c.w), np.uint8)
                    emu.generate(c.shape, mode, c.w, c.h, c.xf, overlap=False, ec_mode=ec, ec_dist=0, y_down=y_down, correct_only=raw, stencil=plain)
                    assert np.argwhere(plain[::-1] != st).tolist() == [[2, 8]]  # (the modern order's byte: the case does tell the two apart)
    assert seen_the_case
    print("device correction on the host, legacy order: %d values and %d stencil bytes, 0 differ" % (values, texels))


def census(e):
    """What a crafted field must hold, from the field itself."""
    f = e.field[..., :3]
    out = {"inf": bool(np.isinf(f).any()), "nan_one": bool((np.isnan(f).sum(axis=2) == 1).any()), "nan_all": bool(np.isnan(f).all(axis=2).any()),
           "neg_zero": bool(((f == 0) & np.signbit(f)).any()), "equalized": bool(((f[..., 0] == f[..., 1]) & (f[..., 0] == f[..., 2])).any())}
    for name, a, b, t in (("h", f[:, 1:], f[:, :-1], e.tx), ("v", f[1:], f[:-1], e.ty), ("d", f[1:, 1:], f[:-1, :-1], e.tx+e.ty)):
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.sort(np.abs(a-b), axis=2)[..., 1]                           # the second largest channel difference: what detectClash compares
        t = np.float32(t)
        for k, v in (("below", np.nextafter(t, np.float32(0))), ("at", t), ("above", np.nextafter(t, np.float32(1)))):
            out[name+"_"+k] = bool((d == v).any())
    return out


def test_crafted_fields_hold_what_they_are_for():
    fields = LC.crafted_fields()
    assert {(e.n, e.w, e.h) for e in fields} == {(n, w, h) for n in (3, 4) for (w, h) in LC.CRAFTED_SIZES}
    assert np.float32(LC.CRAFTED_TX) == LC.CRAFTED_TX and np.float32(LC.CRAFTED_TY) == LC.CRAFTED_TY and np.float32(LC.CRAFTED_TX+LC.CRAFTED_TY) == LC.CRAFTED_TX+LC.CRAFTED_TY
    for e in fields:
        got = census(e)
        if min(e.w, e.h) >= 9:
            assert all(got.values()), (e.n, e.w, e.h, got)
        elif (e.w, e.h) == (2, 2):
            assert got["h_at"] and got["v_at"] and got["inf"] and got["nan_one"] and got["neg_zero"], got
        else:
            assert got["inf"] and got["nan_one"] and got["neg_zero"], got
        assert (e.field == -np.finfo(np.float32).max).any() or min(e.w, e.h) < 9
    # the recorded fixture holds these very fields
    for e, g in zip(fields, LC.crafted_golden()):
        assert (e.n, e.w, e.h, e.tx, e.ty) == (g.n, g.w, g.h, g.tx, g.ty) and LC.differing(e.field, g.field) == 0
        assert np.array_equal(np.signbit(e.field), np.signbit(g.field))


def test_host_clash_passes_on_crafted_fields_equal_the_recorded_reference(host):
    changed = 0
    for e in LC.crafted_golden():
        got = LC.host_correction(host, e.field, e.tx, e.ty)
        assert LC.differing(got, e.out) == 0, (e.n, e.w, e.h)
        if e.n == 4:
            assert LC.differing(got[..., 3], e.field[..., 3]) == 0
        changed += LC.differing(e.out, e.field)
    assert changed > 0


def test_host_clash_passes_on_crafted_fields_equal_the_compiled_reference(rl, host):
    for e in LC.crafted_golden():
        want = rl.correction(e.field, e.tx, e.ty)
        assert LC.differing(want, e.out) == 0, ("recorded", e.n, e.w, e.h)
        assert LC.differing(LC.host_correction(host, e.field, e.tx, e.ty), want) == 0, (e.n, e.w, e.h)
