"""The micro-batcher's group planner without a GPU: the host-only header msdfgen_amd/csrc/msdf_groupplan.hpp (which queued calls may share a group, which of
them a leader takes, the packed layout of a group of different sizes, the index arithmetic of k_boxes_to_slots; compiled with the host compiler from
tests/groupplan_host) on hand-computed cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from msdfgen_amd import lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "groupplan_host", "groupplan_host.cpp")
BOXES = [(1, 1), (7, 9), (8, 8), (9, 8), (8, 9), (24, 1), (1, 17), (23, 17), (16, 16), (17, 10), (24, 17)]     # the boxes of tests/test_gpu_sized.py
TEXELS = 1+63+64+72+72+24+17+391+256+170+408
LIMIT = 256 << 20                                                           # GROUP_BYTES_LIMIT of msdf_capi.hip
i32, i64, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("groupplan_host")), "groupplan_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", SRC, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.group_compatible.argtypes = [i32, C.c_void_p, i32, C.c_void_p, C.c_ulonglong]
    lib.group_select.argtypes = [C.c_int, i32, C.c_int, C.c_int, C.c_ulonglong, C.c_double, u8, C.POINTER(C.c_longlong)]
    lib.group_select.restype = None
    lib.group_packed_offsets.argtypes = [C.c_int, i32, C.c_int, i64]
    lib.group_packed_offsets.restype = None
    lib.box_chunk.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.boxes_to_slots.argtypes = [C.c_int, i32, C.c_int, C.c_longlong, i64, C.POINTER(C.c_float), C.c_longlong, C.POINTER(C.c_float), u8]
    lib.boxes_to_slots.restype = C.c_longlong
    return lib


def select(host, sizes, channels=3, cap=256, limit=LIMIT, max_pad=5.):
    a = np.ascontiguousarray(sizes, np.int32).reshape(-1)
    n = len(a)//2
    taken = np.full(n, 9, np.uint8)
    out = (C.c_longlong*6)()
    host.group_select(n, a.ctypes.data_as(i32), channels, cap, limit, max_pad, taken.ctypes.data_as(u8), out)
    d = dict(zip(("n", "W", "H", "slot", "box_texels", "uniform"), (int(v) for v in out)))
    assert set(taken.tolist()) <= {0, 1} and int(taken.sum()) == d["n"] and taken[0] == 1
    return taken.tolist(), d


def offsets(host, sizes, channels):
    a = np.ascontiguousarray(sizes, np.int32).reshape(-1)
    off = np.zeros(len(a)//2+1, np.int64)
    host.group_packed_offsets(len(a)//2, a.ctypes.data_as(i32), channels, off.ctypes.data_as(i64))
    return off.tolist()


def test_equal_sizes_are_uniform_and_keep_the_layout_of_today(host):
    for pad in (0., 5., 1000.):
        taken, d = select(host, [(16, 16)]*7, max_pad=pad)
        assert taken == [1]*7 and d == {"n": 7, "W": 16, "H": 16, "slot": 256, "box_texels": 7*256, "uniform": 1}
    # tiles one after the other, g*w*h*channels -- already multiples of 4 here; a 5 x 5 tile of one channel (25 floats) is rounded up to 28
    assert offsets(host, [(16, 16)]*3, 3) == [0, 768, 1536, 2304]
    assert offsets(host, [(5, 5)]*3, 1) == [0, 28, 56, 84]
    assert offsets(host, [], 3) == [0]
    taken, d = select(host, [(64, 64)])
    assert taken == [1] and d["uniform"] == 1 and (d["n"], d["slot"]) == (1, 4096)


def test_the_box_cycle(host):
    taken, d = select(host, BOXES, max_pad=1000.)
    assert taken == [1]*11 and d == {"n": 11, "W": 24, "H": 17, "slot": 408, "box_texels": TEXELS, "uniform": 0}
    taken, d = select(host, BOXES*2, max_pad=1000.)
    assert d["n"] == 22 and d["box_texels"] == 2*TEXELS and d["slot"] == 408
    # by hand: the float counts w*h*N, each rounded up to a multiple of 4, summed
    assert offsets(host, BOXES, 1) == [0, 4, 68, 132, 204, 276, 300, 320, 712, 968, 1140, 1548]
    assert offsets(host, BOXES, 3) == [0, 4, 196, 388, 604, 820, 892, 944, 2120, 2888, 3400, 4624]
    assert offsets(host, BOXES, 4) == [0, 4, 256, 512, 800, 1088, 1184, 1252, 2816, 3840, 4520, 6152]
    for n in (1, 3, 4):
        assert all(v % 4 == 0 for v in offsets(host, BOXES, n))


def test_w_and_h_may_come_from_different_calls(host):
    taken, d = select(host, [(30, 2), (3, 40), (5, 5)], max_pad=1000.)
    assert taken == [1, 1, 1] and (d["W"], d["H"], d["slot"], d["box_texels"], d["uniform"]) == (30, 40, 1200, 60+120+25, 0)


def test_selection_by_padding(host):
    big, small = (64, 64), (8, 8)
    # 2*4096 = 8192 > 1.5*(4096+64) = 6240: the leader alone, every small call passed over
    taken, d = select(host, [big]+[small]*10, max_pad=1.5)
    assert taken == [1]+[0]*10 and d["n"] == 1 and d["uniform"] == 1
    # at 2 the bound on the whole group would admit the PAIR (2*max <= 2*(max+min): 8192 <= 8320); the bound on every member does not: 4096 > 2*64
    taken, d = select(host, [big]+[small]*10, max_pad=2.)
    assert taken == [1]+[0]*10 and (d["n"], d["slot"], d["box_texels"], d["uniform"]) == (1, 4096, 4096, 1)
    # the large one last: ten equal calls (padding 1), then 11*4096 = 45056 > 2*(640+4096) = 9472
    for pad in (1.5, 2.):
        taken, d = select(host, [small]*10+[big], max_pad=pad)
        assert taken == [1]*10+[0] and d == {"n": 10, "W": 8, "H": 8, "slot": 64, "box_texels": 640, "uniform": 1}
    taken, d = select(host, [small]*10+[big], max_pad=1000.)
    assert taken == [1]*11 and d["slot"] == 4096
    # a call passed over does not end the walk: what fits behind it is still taken
    taken, d = select(host, [small, big, small, (9, 8), big, small], max_pad=1.5)
    assert taken == [1, 0, 1, 1, 0, 1] and (d["W"], d["H"], d["n"]) == (9, 8, 4)            # 4*72 = 288 <= 1.5*264 = 396
    # the comparison is <=: a slot of exactly maxPad times the smallest box
    assert select(host, [(4, 4), (4, 2), (4, 2)], max_pad=2.)[0] == [1, 1, 1]                  # 16 <= 2*8
    assert select(host, [(4, 4), (4, 2), (4, 2)], max_pad=1.99)[0] == [1, 0, 0]
    assert select(host, [(4, 4), (4, 3)], max_pad=4/3)[0] == [1, 1]                            # 16 <= (4/3)*12 = 16 in fp64
    assert select(host, [(4, 4), (4, 3)], max_pad=1.3)[0] == [1, 0]


def test_every_member_is_bounded_whichever_arrived_first(host):
    """No call sits in a slot of more than maxPad times its own box: the same two kinds are kept apart in either arrival order, a small call that arrived
    early keeps a large one out, and a call that only raises W next to one that only raises H is judged by the slot the two make together."""
    for pad in (2., 5., 63.9):
        assert select(host, [(64, 64)]+[(8, 8)]*10, max_pad=pad)[0] == [1]+[0]*10, pad
        assert select(host, [(8, 8)]*10+[(64, 64)], max_pad=pad)[0] == [1]*10+[0], pad
    assert select(host, [(64, 64)]+[(8, 8)]*10, max_pad=64.)[0] == [1]*11                      # 4096 <= 64*64, and 11*4096 <= 64*4736
    assert select(host, [(8, 8)]*10+[(64, 64)], max_pad=64.)[0] == [1]*11
    assert select(host, [(16, 16), (4, 4), (16, 16)], max_pad=4.)[0] == [1, 0, 1]
    assert select(host, [(4, 4), (16, 16), (4, 4)], max_pad=4.)[0] == [1, 0, 1]
    taken, d = select(host, [(20, 10), (10, 20), (20, 10)], max_pad=2.)                        # 20 x 20 = 400 <= 2*200
    assert taken == [1, 1, 1] and d["slot"] == 400
    assert select(host, [(20, 10), (10, 20), (20, 10)], max_pad=1.9)[0] == [1, 0, 1]
    # what the member bound implies for the group: n*slot <= maxPad*sum of w*h in every selection
    rng = np.random.default_rng(11)
    for pad in (1.5, 3., 5.):
        sizes = rng.integers(1, 40, (200, 2))
        taken, d = select(host, sizes, max_pad=pad)
        assert d["n"]*d["slot"] <= pad*d["box_texels"] and d["slot"] <= pad*min(int(w)*int(h) for (w, h), t in zip(sizes, taken) if t)


def test_max_pad_below_one_means_equal_sizes(host):
    calls = [(8, 8), (9, 8), (8, 8), (8, 9), (8, 8), (1, 1)]
    for pad in (0., .5, .999, -3., float("nan")):
        taken, d = select(host, calls, max_pad=pad)
        assert taken == [1, 0, 1, 0, 1, 0] and d == {"n": 3, "W": 8, "H": 8, "slot": 64, "box_texels": 192, "uniform": 1}, pad
    taken, d = select(host, calls, max_pad=1.)                                                 # 1: no padding at all -- equal sizes again, by the comparison
    assert taken == [1, 0, 1, 0, 1, 0] and d["uniform"] == 1


def test_cap_and_byte_limit(host):
    taken, d = select(host, BOXES*3, cap=5, max_pad=1000.)
    assert taken == [1]*5+[0]*28 and d["n"] == 5
    taken, d = select(host, [(16, 16)]*9, cap=4, max_pad=0.)
    assert taken == [1]*4+[0]*5
    assert select(host, [(16, 16)]*3, cap=1)[0] == [1, 0, 0]
    # the leader is taken even when it alone exceeds the byte limit; nothing joins it
    taken, d = select(host, [(64, 64), (64, 64), (1, 1)], limit=1000, max_pad=1000.)
    assert taken == [1, 0, 0] and d["slot"] == 4096
    # the limit counts n*W*H*channels*4, not the boxes: 3 slots of 64 x 64 x 3 floats = 147 456 B
    taken, d = select(host, [(64, 64), (1, 1), (1, 1), (1, 1)], limit=147456, max_pad=4096.)
    assert taken == [1, 1, 1, 0]
    taken, d = select(host, [(64, 64), (1, 1), (1, 1), (1, 1)], limit=147455, max_pad=4096.)
    assert taken == [1, 1, 0, 0]
    # ... and grows when a later call raises W or H: (1, 1) x 3 fit in any limit, the 64 x 64 behind them would make four slots of 49 152 B
    taken, d = select(host, [(1, 1), (1, 1), (1, 1), (64, 64), (2, 2)], limit=150000, max_pad=1e9)
    assert taken == [1, 1, 1, 0, 1] and (d["W"], d["H"]) == (2, 2)
    # equal sizes under the limit exactly as before sizes could differ: n*tileBytes <= limit
    taken, d = select(host, [(64, 64)]*6, limit=4*49152, max_pad=0.)
    assert taken == [1]*4+[0]*2
    assert select(host, [(64, 64)]*6, limit=4*49152, max_pad=5.)[0] == [1]*4+[0]*2


def test_the_texel_index_bound_is_that_of_the_sized_plan(host):
    """n*slot must stay below SIZED_MAX_SLOT_TEXELS (2^32-1, msdf_sizedplan.hpp: asked through sizedLayout): 15 slots of 16 384 x 16 384 (2^28 texels) fit, the
    16th is one too many -- with a byte limit that would allow either --, and sides of 2^31-1 are refused without an overflow on the way."""
    huge = 2**64-1
    boxes = np.full((17, 2), 1 << 14)
    boxes[1, 1] -= 1                                                       # (two sizes: a group of equal sizes runs without sizes and is not asked)
    taken, d = select(host, boxes[:15], limit=huge, max_pad=1000.)
    assert taken == [1]*15 and d["n"]*d["slot"] == 0xf0000000 and d["uniform"] == 0
    taken, d = select(host, boxes, limit=huge, max_pad=1000.)
    assert taken == [1]*15+[0, 0] and d["n"] == 15
    assert select(host, np.full((17, 2), 1 << 14), limit=huge, max_pad=1000.)[0] == [1]*17   # equal sizes: as before sizes could differ
    taken, d = select(host, [(0x7fffffff, 0x7fffffff)]*2, cap=256, limit=huge, max_pad=1000.)
    assert taken == [1, 0] and d["slot"] == 0x7fffffff**2
    taken, d = select(host, [(1 << 16, 1), (1, 1 << 16)], limit=huge, max_pad=1e12)
    assert taken == [1, 0]
    taken, d = select(host, [(1, 1), (0x7fffffff, 0x7fffffff), (1, 1)], limit=LIMIT, max_pad=1e30)
    assert taken == [1, 0, 1]


def test_compatibility(host):
    cfg = L.Config(1, 2, 1, 0, 1.1, 1.1, 0, 0, .5, 0)
    legacy = host.group_legacy_op()
    assert legacy == 4 and [host.group_op_takes_sizes(op) for op in range(5)] == [1, 1, 1, 1, 0]

    def ok(a, b, cfg_b=cfg):
        ka, kb = (C.c_int32*5)(*a), (C.c_int32*5)(*b)
        return bool(host.group_compatible(ka, C.addressof(cfg), kb, C.addressof(cfg_b), C.sizeof(L.Config)))
    for op in range(4):                                                     # generate, error correction, sign correction, rasterize: sizes may differ
        assert ok((3, 3, op, 24, 17), (3, 3, op, 24, 17)) and ok((3, 3, op, 24, 17), (3, 3, op, 7, 9))
        assert not ok((3, 3, op, 24, 17), (4, 3, op, 24, 17)) and not ok((3, 3, op, 24, 17), (3, 4, op, 24, 17))
        assert not ok((3, 3, op, 24, 17), (3, 3, (op+1) % 4, 24, 17))
    assert ok((3, 3, legacy, 24, 17), (3, 3, legacy, 24, 17))              # the legacy generators: never two sizes in one group
    assert not ok((3, 3, legacy, 24, 17), (3, 3, legacy, 24, 16)) and not ok((3, 3, legacy, 24, 17), (3, 3, legacy, 23, 17))
    assert not ok((3, 3, legacy, 24, 17), (3, 3, 0, 24, 17))
    for field, value in (("overlap_support", 0), ("ec_mode", 1), ("ec_distance_check", 2), ("ec_stage_limit", 1), ("min_deviation_ratio", 1.2),
                         ("min_improve_ratio", 1.2), ("sign_correction", 1), ("fill_rule", 1), ("sdf_zero_value", .25), ("stencil_y_down", 1)):
        other = L.Config.from_buffer_copy(cfg)
        setattr(other, field, value)
        assert not ok((3, 3, 0, 24, 17), (3, 3, 0, 24, 17), other), field   # the whole config is part of the key


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_boxes_to_slots_index_function_against_a_plain_copy(host, channels):
    """k_boxes_to_slots' grid walked on the host over two turns of BOXES (boxes whose float count is no multiple of 4, the 1 x 1 box, the box that fills its
    slot; slots that start off a 16-byte boundary: 408*1 and 408*3 floats are multiples of 4, so a 23 x 17 slot is walked as well)."""
    for sizes in (BOXES*2, [b for b in BOXES if b != (24, 17)]*2):
        a = np.ascontiguousarray(sizes, np.int32)
        n, slot = len(a), int(a[:, 0].max())*int(a[:, 1].max())
        off = np.array(offsets(host, a, channels), np.int64)
        rng = np.random.default_rng(7)
        packed = rng.random(int(off[-1]), np.float32)
        dst = np.full(n*slot*channels, -1, np.float32)
        writes = np.zeros(dst.size, np.uint8)
        rc = host.boxes_to_slots(n, a.ctypes.data_as(i32), channels, slot, off.ctypes.data_as(i64), packed.ctypes.data_as(C.POINTER(C.c_float)), packed.size,
                                 dst.ctypes.data_as(C.POINTER(C.c_float)), writes.ctypes.data_as(u8))
        assert rc == 0
        want, once = np.full_like(dst, -1), np.zeros_like(writes)
        for g, (w, h) in enumerate(a.tolist()):                             # the plain per-box copy
            f = w*h*channels
            want[g*slot*channels:g*slot*channels+f] = packed[off[g]:off[g]+f]
            once[g*slot*channels:g*slot*channels+f] = 1
        assert (dst.view(np.uint32) == want.view(np.uint32)).all() and (writes == once).all()
    # single chunks: a full one, the partial tail of a 7 x 9 x 3 box (189 floats = 47 chunks + 1 float), the first chunk beyond
    s, d = C.c_longlong(), C.c_longlong()
    assert host.box_chunk(7, 9, 3, 4, 1224, 1, 0, C.byref(s), C.byref(d)) == 4 and (s.value, d.value) == (4, 1224)
    assert host.box_chunk(7, 9, 3, 4, 1224, 1, 47, C.byref(s), C.byref(d)) == 1 and (s.value, d.value) == (4+188, 1224+188)
    assert host.box_chunk(7, 9, 3, 4, 1224, 1, 48, C.byref(s), C.byref(d)) == 0
    assert host.box_chunk(1, 1, 1, 0, 408, 0, 0, C.byref(s), C.byref(d)) == 1 and host.box_chunk(1, 1, 1, 0, 408, 0, 1, C.byref(s), C.byref(d)) == 0


def test_sanitized_build_of_the_host_program(tmp_path):
    """The header under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program (host code only). Skipped only where an EMPTY program
    cannot be built with those flags."""
    from test_ec_lazy_host import _sanitizers_link
    if not _sanitizers_link(tmp_path):
        pytest.skip("g++ cannot build an empty program with -fsanitize=address,undefined here")
    exe = os.path.join(str(tmp_path), "groupplan_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGROUPPLAN_MAIN", SRC, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr[-2000:])
