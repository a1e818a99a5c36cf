"""msdfhip_batch_gather without a GPU: the host-only header msdfgen_amd/csrc/msdf_gatherplan.hpp (validation, 64-bit totals, maxima of the selection, the
table of exclusive prefix sums; compiled with the host compiler from tests/gatherplan_host) on hand-computed cases, and the refusals of the C entry point that
are returned before any source batch is read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from msdfgen_amd import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gatherplan_host", "gatherplan_host.cpp")
CODES = ("ok", "no_sources", "bad_count", "no_indices", "no_source_of", "bad_source", "bad_index", "mixed_devices", "too_many_contours", "too_many_edges")
INT32_MAX = 2**31-1

# (contours, edges) per glyph. FONT_A has an empty glyph in the middle and one at the end, FONT_B has other counts.
FONT_A = [(2, 7), (0, 0), (1, 3), (4, 40), (0, 0)]
FONT_B = [(3, 9), (1, 4)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("gatherplan_host")), "gatherplan_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    lib = C.CDLL(so)
    ip, i32, ll = C.POINTER(C.c_int), C.POINTER(C.c_int32), C.POINTER(C.c_longlong)
    lib.gather_plan.argtypes = [C.c_int, ip, ip, ip, ip, C.c_int, i32, i32, ll, ll, ll, i32, ip, ip]
    return lib


def plan(host, fonts, source_of, indices, devices=None, n_glyphs=None, n_sources=None, fill=True):
    """Runs the plan over `fonts` (lists of (contours, edges) per glyph; None: "sources is NULL"). Returns (code name, refusal, totals, table columns, counts)."""
    code = {host.gather_codes(k): name for k, name in enumerate(CODES)}
    assert len(code) == len(CODES) and host.gather_codes(0) == 0
    ip, i32 = C.POINTER(C.c_int), C.POINTER(C.c_int32)
    as_int = lambda a: np.ascontiguousarray(a, np.intc)
    if fonts is None:
        n_of = dev = contours = edges = None
    else:
        n_of = as_int([len(f) for f in fonts])
        dev = as_int(devices if devices is not None else [0]*len(fonts))
        flat = [ce for f in fonts for ce in f]
        contours, edges = as_int([c for c, _ in flat]+[0]), as_int([e for _, e in flat]+[0])
    idx = None if indices is None else np.ascontiguousarray(indices, np.int32)
    src = None if source_of is None else np.ascontiguousarray(source_of, np.int32)
    n = (0 if idx is None else len(idx)) if n_glyphs is None else n_glyphs
    refusal, totals, columns = (C.c_longlong*3)(), (C.c_longlong*4)(), (C.c_longlong*7)()
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    call = lambda table, sc, se: host.gather_plan(len(fonts or []) if n_sources is None else n_sources, p(n_of, ip), p(dev, ip), p(contours, ip), p(edges, ip), n,
                                                  p(src, i32), p(idx, i32), refusal, totals, columns, p(table, i32), p(sc, ip), p(se, ip))
    rc = call(None, None, None)
    out = {"refusal": tuple(int(v) for v in refusal), "totals": tuple(int(v) for v in totals)}
    if rc == 0 and fill:
        names = ("dst_contour0", "source", "src_glyph", "src_contour0", "src_edge0", "dst_edge0")
        col = dict(zip(names, (int(v) for v in columns)))
        table = np.full(int(columns[6]), -7, np.int32)
        sc, se = np.full(max(n, 1), -7, np.intc), np.full(max(n, 1), -7, np.intc)
        assert call(table, sc, se) == 0
        out["table"] = {k: table[col[k]:col[k]+n+(1 if k in ("dst_contour0", "dst_edge0") else 0)].tolist() for k in names}
        out["counts"] = (sc[:n].tolist(), se[:n].tolist())
        used = np.zeros(len(table), bool)
        for k in names:
            used[col[k]:col[k]+n+(1 if k in ("dst_contour0", "dst_edge0") else 0)] = True
        assert (table[~used] == 0).all() and int(columns[6]) % 4 == 0 and col["source"] % 4 == 0 and col["dst_contour0"] == 0     # padding zeroed, uploads aligned
    return code[rc], out


def test_table_of_a_selection_with_repeats_and_empty_glyphs(host):
    # FONT_A starts: contours 0, 2, 2, 3, 7 | edges 0, 7, 7, 10, 50
    rc, p = plan(host, [FONT_A], None, [4, 3, 3, 0, 1, 4, 3])
    assert rc == "ok" and p["totals"] == (14, 127, 4, 40)
    assert p["table"] == {"dst_contour0": [0, 0, 4, 8, 10, 10, 10, 14], "dst_edge0": [0, 0, 40, 80, 87, 87, 87, 127], "source": [0]*7,
                          "src_glyph": [4, 3, 3, 0, 1, 4, 3], "src_contour0": [7, 3, 3, 0, 2, 7, 3], "src_edge0": [50, 10, 10, 0, 7, 50, 10]}
    assert p["counts"] == ([0, 4, 4, 2, 0, 0, 4], [0, 40, 40, 7, 0, 0, 40])
    # the identity is the source's own offsets, and the maxima are the SELECTION's, not the source's
    rc, p = plan(host, [FONT_A], None, range(5))
    assert rc == "ok" and p["totals"] == (7, 50, 4, 40) and p["table"]["dst_contour0"] == [0, 2, 2, 3, 7, 7] and p["table"]["dst_edge0"] == [0, 7, 7, 10, 50, 50]
    assert p["table"]["src_contour0"] == p["table"]["dst_contour0"][:5] and p["table"]["src_edge0"] == p["table"]["dst_edge0"][:5]
    rc, p = plan(host, [FONT_A], None, [2, 0, 2])
    assert rc == "ok" and p["totals"] == (4, 13, 2, 7)
    # an explicit source_of of zeros is the same plan
    assert plan(host, [FONT_A], [0, 0, 0], [2, 0, 2]) == (rc, p)


def test_two_sources_with_different_counts(host):
    rc, p = plan(host, [FONT_A, FONT_B], [1, 0, 0, 1, 0], [1, 2, 1, 0, 0])
    assert rc == "ok" and p["totals"] == (7, 23, 3, 9)
    assert p["table"] == {"dst_contour0": [0, 1, 2, 2, 5, 7], "dst_edge0": [0, 4, 7, 7, 16, 23], "source": [1, 0, 0, 1, 0], "src_glyph": [1, 2, 1, 0, 0],
                          "src_contour0": [3, 2, 2, 0, 0], "src_edge0": [9, 7, 7, 0, 0]}
    assert p["counts"] == ([1, 1, 0, 3, 2], [4, 3, 0, 9, 7])
    # the same index means another glyph in another source
    rc, p = plan(host, [FONT_A, FONT_B], [0, 1], [1, 1])
    assert rc == "ok" and p["totals"] == (1, 4, 1, 4) and p["table"]["src_edge0"] == [7, 9]
    # a source nobody selects from is not read: only FONT_B's counts matter here
    rc, p = plan(host, [FONT_A, FONT_B], [1, 1, 1], [0, 0, 1])
    assert rc == "ok" and p["totals"] == (7, 22, 3, 9) and p["table"]["dst_edge0"] == [0, 9, 18, 22]


def test_empty_selection_and_empty_glyphs_only(host):
    rc, p = plan(host, [FONT_A], None, [])
    assert rc == "ok" and p["totals"] == (0, 0, 0, 0) and p["table"]["dst_contour0"] == [0] and p["table"]["dst_edge0"] == [0] and p["counts"] == ([], [])
    rc, p = plan(host, [FONT_A], None, None, n_glyphs=0)                                          # indices may be NULL when nothing is selected
    assert rc == "ok" and p["table"]["dst_contour0"] == [0]
    rc, p = plan(host, [FONT_A], None, [1, 4, 1])
    assert rc == "ok" and p["totals"] == (0, 0, 0, 0) and p["table"]["dst_contour0"] == [0, 0, 0, 0] and p["table"]["src_contour0"] == [2, 7, 2]
    rc, p = plan(host, [[]], None, [])                                                            # a source without glyphs
    assert rc == "ok" and p["totals"] == (0, 0, 0, 0)


def test_refuses_missing_sources(host):
    assert plan(host, None, None, [0], n_sources=1)[0] == "no_sources"
    assert plan(host, [FONT_A], None, [0], n_sources=0)[0] == "no_sources"
    assert plan(host, [FONT_A], None, [0], n_sources=-2)[0] == "no_sources"


def test_refuses_a_negative_glyph_count(host):
    assert plan(host, [FONT_A], None, [0], n_glyphs=-1)[0] == "bad_count"


def test_refuses_missing_indices(host):
    rc, p = plan(host, [FONT_A], None, None, n_glyphs=3)
    assert rc == "no_indices" and p["refusal"][0] == -1


def test_refuses_a_missing_source_of_with_several_sources(host):
    assert plan(host, [FONT_A, FONT_B], None, [0, 1])[0] == "no_source_of"
    assert plan(host, [FONT_A, FONT_B], None, [], n_glyphs=0)[0] == "no_source_of"                # ... whatever is selected


@pytest.mark.parametrize("bad", [2, -1, 7, -2**31])
def test_refuses_a_source_of_outside_the_sources(host, bad):
    rc, p = plan(host, [FONT_A, FONT_B], [0, 1, 1, bad, 0], [0, 0, 1, 0, 9])                      # (the bad index behind it is not reached)
    assert rc == "bad_source" and p["refusal"] == (3, bad, 2)


@pytest.mark.parametrize("bad", [5, -1, 2**31-1])
def test_refuses_an_index_outside_its_source(host, bad):
    rc, p = plan(host, [FONT_A], None, [0, 4, bad, 1])
    assert rc == "bad_index" and p["refusal"] == (2, bad, 5)
    # the bound is the glyph count of the glyph's OWN source: 2 and 4 are fine in FONT_A, not in FONT_B
    rc, p = plan(host, [FONT_A, FONT_B], [0, 0, 1, 1], [2, 4, 1, 2])
    assert rc == "bad_index" and p["refusal"] == (3, 2, 2)
    assert plan(host, [[]], None, [0])[0] == "bad_index"


def test_refuses_sources_on_different_devices(host):
    rc, p = plan(host, [FONT_A, FONT_B, FONT_B], [0, 1, 2], [0, 0, 0], devices=[1, 1, 3])
    assert rc == "mixed_devices" and p["refusal"] == (2, 3, 1)
    assert plan(host, [FONT_A, FONT_B, FONT_B], [0, 1, 2], [0, 0, 0], devices=[1, 1, 1])[0] == "ok"


def test_totals_in_64_bits(host):
    """Instancing reaches INT32_MAX long before the index arrays do: one glyph of 2^20 edges taken 2 048 times is one edge too many, 2 047 times fits."""
    big = [[(1, 1 << 20)]]
    rc, p = plan(host, big, None, np.zeros(2048, np.int32), fill=False)
    assert rc == "too_many_edges" and p["refusal"] == (2047, 1 << 31, INT32_MAX)
    rc, p = plan(host, big, None, np.zeros(2047, np.int32))
    assert rc == "ok" and p["totals"] == (2047, 2047 << 20, 1, 1 << 20) and p["table"]["dst_edge0"][-1] == 2047 << 20 and p["table"]["dst_edge0"][1] == 1 << 20
    # the same for contours, and no wrap-around far beyond the bound
    many = [[(1 << 20, 1 << 20), (3, 1)]]
    rc, p = plan(host, many, None, [1]+[0]*2048, fill=False)
    assert rc == "too_many_contours" and p["refusal"] == (2048, (1 << 31)+3, INT32_MAX)
    rc, p = plan(host, [[(5, INT32_MAX)]], None, np.zeros(5000, np.int32), fill=False)
    assert rc == "too_many_edges" and p["refusal"] == (1, 2*INT32_MAX, INT32_MAX)
    assert plan(host, [[(5, INT32_MAX)]], None, [0], fill=False)[0] == "ok"


def test_c_abi_refuses_bad_arguments_before_any_source_is_read():
    """The refusals of msdfhip_batch_gather that need no batch (only a device can create one): the source pointers below are never dereferenced, the call must
    fail first. Those that read a source's glyph count are in tests/test_gpu_batch_gather.py."""
    lib = L.load()
    assert "msdfhip_batch_gather" in L.EXPORTED_SYMBOLS
    out = C.c_void_p()
    fake = (C.c_void_p*2)(64, 64)
    some = (C.c_void_p*2)(64, None)
    idx = np.zeros(4, np.int32)
    ip = C.POINTER(C.c_int32)
    err = lambda: lib.msdfhip_last_error()
    assert lib.msdfhip_batch_gather(None, fake, 1, 0, None, None, None) == L.ERR_INVALID and b"batch is NULL" in err()
    assert lib.msdfhip_batch_gather(C.byref(out), None, 1, 0, None, None, None) == L.ERR_INVALID and b"no sources" in err()
    assert lib.msdfhip_batch_gather(C.byref(out), fake, 0, 0, None, None, None) == L.ERR_INVALID and b"no sources" in err()
    assert lib.msdfhip_batch_gather(C.byref(out), fake, -3, 0, None, None, None) == L.ERR_INVALID and b"no sources" in err()
    assert lib.msdfhip_batch_gather(C.byref(out), fake, 1, -1, None, idx.ctypes.data_as(ip), None) == L.ERR_INVALID and b"n_glyphs is negative" in err()
    assert lib.msdfhip_batch_gather(C.byref(out), fake, 1, 4, None, None, None) == L.ERR_INVALID and b"indices is NULL" in err()
    assert lib.msdfhip_batch_gather(C.byref(out), fake, 2, 4, None, idx.ctypes.data_as(ip), None) == L.ERR_INVALID and b"source_of is NULL" in err()
    assert lib.msdfhip_batch_gather(C.byref(out), some, 2, 4, idx.ctypes.data_as(ip), idx.ctypes.data_as(ip), None) == L.ERR_INVALID and b"sources[1] is NULL" in err()
    assert not out.value
    assert lib.msdfhip_abi_version() == 5


def test_sanitized_build_of_the_host_program(tmp_path):
    """The header under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program (host code only). Skipped only where an EMPTY program
    cannot be built with those flags."""
    from test_ec_lazy_host import _sanitizers_link
    if not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    exe = os.path.join(str(tmp_path), "gatherplan_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGATHERPLAN_MAIN", SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])
