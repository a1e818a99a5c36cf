"""The end-to-end host-memory path (msdfhip_batch_generate_host / _bytes_host: chunked two-stream pipeline), per-batch device binding
and the glyph-sharded multi-device generator (msdfhip_generate_sharded), through the C ABI on a real MI355X.  Everything here is
byte-exact by construction (same kernels, different plumbing), so the assertions are on bits."""
import ctypes as C
import threading

import numpy as np
import pytest

import msdfgen_amd as M
from conftest import load_npz, bits
from msdfgen_amd import lib as L
from msdfgen_amd.shape import ShapeBatch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    M.init(0)


@pytest.fixture(scope="module")
def glyphs():
    """1 500 distinct DejaVu glyphs (every fifth of the config-4 fixture: mixes 1..43 contours) + their 48x48 frames and reference hashes."""
    z = load_npz("dejavu8192.npz")
    full = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                      z["colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    idx = list(range(0, 7500, 5))
    sub = full.select(idx)
    want = M.GlyphBatch(sub).generate(M.MODE_MSDF, 48, 48, z["xf48"][idx]).cpu().numpy()
    # `want` is what every test of this module compares the plumbing with -- itself pinned here to the compiled REFERENCE's sha256 per tile (the fixture's
    # sha48, tools/make_golden_full.py), so that a defect common to the device batch and the pipelines cannot pass unnoticed.
    import hashlib
    for k, g in enumerate(idx):
        assert (np.frombuffer(hashlib.sha256(np.ascontiguousarray(want[k]).tobytes()).digest(), np.uint8) == z["sha48"][g]).all(), (g, sub.names[k])
    return sub, z["xf48"][idx], want


def test_host_pipeline_packed_matches_device_batch(glyphs):
    sub, xfs, want = glyphs
    hb = M.HostBatch(sub)
    try:
        for chunk in (0, 256, 1000, 4096):                                    # automatic; several chunks + a ragged last one; one chunk
            L.load().msdfhip_set_pipeline_chunk(chunk)
            out = M.host_alloc((sub.n_glyphs, 48, 48, 3))
            out[:] = 7
            st = np.zeros((sub.n_glyphs, 48, 48), np.uint8)
            hb.generate_host(M.MODE_MSDF, 48, 48, xfs, out=out, stencil=st)
            assert (bits(out) == bits(want)).all(), "chunk %d" % chunk
            assert st.any() and ((st & np.uint8(0xfc)) == 0).all()
            M.host_free(out)
        out = hb.generate_host(M.MODE_MSDF, 48, 48, xfs)                      # pageable output
        assert (bits(out) == bits(want)).all()
        sdf = hb.generate_host(M.MODE_SDF, 48, 48, xfs)
        assert (bits(sdf) == bits(M.GlyphBatch(sub).generate(M.MODE_SDF, 48, 48, xfs).cpu().numpy())).all()
    finally:
        L.load().msdfhip_set_pipeline_chunk(0)
        hb.close()


def test_host_pipeline_atlas_rectangles_preserve_the_rest(glyphs):
    """Tiles as rectangles of one larger float atlas (BitmapSection of a bigger bitmap, core/BitmapRef.hpp:74-111), every second glyph
    with a negative row stride (bottom-up rows); texels outside the rectangles keep the caller's values."""
    sub, xfs, want = glyphs
    n = 600
    part = sub.select(list(range(n)))
    cols = 25
    rows = (n+cols-1)//cols
    pad = 3
    aw, ah = cols*(48+pad), rows*(48+pad)
    atlas = np.full((ah, aw, 3), -5., np.float32)
    offs, strides = np.zeros(n, np.int64), np.zeros(n, np.int32)
    for g in range(n):
        x0, y0 = (g % cols)*(48+pad)+1, (g//cols)*(48+pad)+2
        if g % 2:
            offs[g], strides[g] = ((y0+47)*aw+x0)*3, -aw*3
        else:
            offs[g], strides[g] = (y0*aw+x0)*3, aw*3
    hb = M.HostBatch(part)
    try:
        L.load().msdfhip_set_pipeline_chunk(128)
        hb.generate_host(M.MODE_MSDF, 48, 48, xfs[:n], out=atlas, out_offsets=offs, row_stride=strides)
    finally:
        L.load().msdfhip_set_pipeline_chunk(0)
        hb.close()
    covered = np.zeros((ah, aw), bool)
    for g in range(n):
        x0, y0 = (g % cols)*(48+pad)+1, (g//cols)*(48+pad)+2
        rect = atlas[y0:y0+48, x0:x0+48]
        tile = want[g][::-1] if g % 2 else want[g]
        assert (bits(rect) == bits(tile)).all(), g
        covered[y0:y0+48, x0:x0+48] = True
    assert (atlas[~covered] == -5.).all()


def test_host_pipeline_overlapping_rectangles_leave_the_gap_alone(glyphs):
    """a chunk whose rectangles have the AREA of a contiguous range but are not disjoint -- two glyphs on one cell of a
    gap-free atlas and one cell nobody writes -- must not take the single-copy path: the free cell keeps the caller's values (it used to
    come back as whatever the device buffer held)."""
    sub, xfs, want = glyphs
    n, cols = 128, 16
    aw = cols*48
    atlas = np.full((n//cols*48, aw, 3), -7., np.float32)
    cell = list(range(n))
    cell[5] = 4                                                           # glyphs 4 and 5 share cell 4; cell 5 stays free
    offs = np.array([((c//cols)*48*aw+(c % cols)*48)*3 for c in cell], np.int64)
    hb = M.HostBatch(sub.select(list(range(n))))
    try:
        L.load().msdfhip_set_pipeline_chunk(128)
        hb.generate_host(M.MODE_MSDF, 48, 48, xfs[:n], out=atlas, out_offsets=offs, row_stride=np.full(n, aw*3, np.int32))
    finally:
        L.load().msdfhip_set_pipeline_chunk(0)
        hb.close()
    for g in range(n):
        c = cell[g]
        rect = atlas[(c//cols)*48:(c//cols)*48+48, (c % cols)*48:(c % cols)*48+48]
        if g == 4:
            assert (bits(rect) == bits(want[4])).all() or (bits(rect) == bits(want[5])).all()   # shared cell: one of the two, whole
        elif g != 5:
            assert (bits(rect) == bits(want[g])).all(), g
    assert (atlas[0:48, 5*48:6*48] == -7.).all(), "the free cell was overwritten"


def test_bytes_pipeline_matches_pixel_float_to_byte(glyphs, oracle):
    sub, xfs, want = glyphs
    n = 1024
    part = sub.select(list(range(n)))
    cols = 32
    aw = cols*48
    atlas = np.full((n//cols*48, aw, 3), 9, np.uint8)
    offs = np.array([((g//cols)*48*aw+(g % cols)*48)*3 for g in range(n)], np.int64)
    hb = M.HostBatch(part)
    try:
        L.load().msdfhip_set_pipeline_chunk(160)
        hb.generate_bytes_host(M.MODE_MSDF, 48, 48, xfs[:n], atlas, offs, aw*3)
        packed = np.zeros((n, 48, 48, 3), np.uint8)                           # byte tiles in glyph order: the per-chunk contiguous copy path
        hb.generate_bytes_host(M.MODE_MSDF, 48, 48, xfs[:n], packed, np.arange(n, dtype=np.int64)*48*48*3, 48*3)
    finally:
        L.load().msdfhip_set_pipeline_chunk(0)
        hb.close()
    ref = oracle.pixel_float_to_byte(want[:n])
    assert (packed == ref).all()
    for g in range(0, n, 7):
        y0, x0 = (g//cols)*48, (g % cols)*48
        assert (atlas[y0:y0+48, x0:x0+48] == ref[g]).all(), g


@pytest.mark.parametrize("chunk,n", [(171, 450), (180, 700), (100, 333), (65, 1500)])
def test_bytes_pipeline_with_chunk_sizes_that_are_not_multiples_of_64(glyphs, oracle, chunk, n):
    """the 8-bit tail schedule rounds its pieces to 64 glyphs; with msdfhip_set_pipeline_chunk(171) and 450 glyphs it scheduled 64, 171, 192, 23 --
    a 192-glyph piece in slots sized for 171 (device tiles, descriptors, pinned staging). Every scheduled piece is now cut to the slot capacity; the resident
    and the streamed pipeline, 8-bit and float, against the device batch."""
    sub, xfs, want = glyphs
    part = sub.select(list(range(n)))
    ref = oracle.pixel_float_to_byte(want[:n])
    offs = np.arange(n, dtype=np.int64)*48*48*3
    lib = L.load()
    hb = M.HostBatch(part)
    try:
        lib.msdfhip_set_pipeline_chunk(chunk)
        packed = np.zeros((n, 48, 48, 3), np.uint8)
        hb.generate_bytes_host(M.MODE_MSDF, 48, 48, xfs[:n], packed, offs, 48*3)
        assert (packed == ref).all()
        a8 = np.zeros((n, 48, 48, 3), np.uint8)
        M.generate_stream(part, M.MODE_MSDF, 48, 48, xfs[:n], atlas=a8, out_offsets=offs, row_stride=48*3)
        assert (a8 == ref).all()
        assert (bits(hb.generate_host(M.MODE_MSDF, 48, 48, xfs[:n])) == bits(want[:n])).all()
        assert (bits(M.generate_stream(part, M.MODE_MSDF, 48, 48, xfs[:n])) == bits(want[:n])).all()
    finally:
        lib.msdfhip_set_pipeline_chunk(0)
        hb.close()


def test_sharded_over_the_same_device_is_byte_identical(glyphs):
    """msdfhip_generate_sharded with the one GPU of the box listed 1, 2 and 5 times: each entry is its own host thread + batch + streams
    (what runs on 8 GPUs with devices = 0..7); the bytes must not depend on the split."""
    sub, xfs, want = glyphs
    assert L.load().msdfhip_device_count is not None
    for devices in ([0], [0, 0], [0, 0, 0, 0, 0]):
        out = M.generate_sharded(devices, sub, M.MODE_MSDF, 48, 48, xfs)
        assert (bits(out) == bits(want)).all(), devices
    atlas = np.zeros((sub.n_glyphs, 48, 48, 3), np.uint8)
    M.generate_sharded([0, 0, 0], sub, M.MODE_MSDF, 48, 48, xfs, atlas=atlas, out_offsets=np.arange(sub.n_glyphs, dtype=np.int64)*48*48*3, row_stride=48*3)
    assert atlas.any()
    with pytest.raises(M.MsdfHipError):
        M.generate_sharded([0, 99], sub, M.MODE_MSDF, 48, 48, xfs)


def test_batch_remembers_its_device(glyphs):
    sub, xfs, want = glyphs
    hb = M.HostBatch(sub.select([0, 1, 2]), device=0)
    assert hb.device == 0
    hb.close()
    with pytest.raises(M.MsdfHipError):
        M.HostBatch(sub.select([0]), device=64)


def test_failed_generate_leaves_nothing_to_the_next_call(glyphs):
    """A call that fails after its distance pass queued the correction pass's k_ec_params on a side stream (1 500 glyphs fork the glyph classes),
    here at the sign pass's fill-rule check, must not change what the next call on the same resident batch computes: its per-glyph
    constants come from its own request.  Same bitmap size in both calls, so every buffer region is in bounds whatever the failed call left."""
    sub, xfs, want = glyphs
    other = np.array(xfs, np.float64, copy=True)
    other[:, :2] *= .9
    other[:, 2:4] += .25
    gb = M.GlyphBatch(sub)
    with pytest.raises(M.MsdfHipError):
        gb.generate(M.MODE_MSDF, 48, 48, other, scanline_pass=True, fill_rule=7)
    got = gb.generate(M.MODE_MSDF, 48, 48, xfs).cpu().numpy()
    assert (bits(got) == bits(want)).all()


def test_device_memory_stays_flat_over_many_calls(glyphs):
    """Long-running callers: single-shape calls mixing few- and many-contour shapes, and fresh worker threads for every
    round (msdf-atlas-gen spawns a new team per Workload::finish()), must not grow device or pinned memory."""
    import torch
    sub, xfs, want = glyphs
    n_c = np.diff(sub.glyph_contour_offsets)
    many = int(np.argmax(n_c))
    assert n_c[many] >= 10
    picks = [many, 0, int(np.argsort(n_c)[-2]), 1]

    def work():
        for g in picks:
            out = np.zeros((48, 48, 3), np.float32)
            M.generate_msdf(out, sub.shape(g), M.SDFTransformation.from_xf(xfs[g]))
            assert (bits(out) == bits(want[g])).all()

    def round_of_threads():
        ts = [threading.Thread(target=work) for _ in range(6)]
        [t.start() for t in ts]
        [t.join() for t in ts]

    for _ in range(8):                                                        # the pool grows to the largest number of calls ever in flight at once (<= 6 here)
        round_of_threads()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(25):
        round_of_threads()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    # a leak of one arena per thread (round 1) would be 150 arenas here; one more pooled arena (a round that happened to overlap more calls
    # than any warm-up round did) is allowed
    assert free0-free1 < 24 << 20, "device memory grew by %.1f MB over 25 rounds of fresh threads" % ((free0-free1)/2**20)


def test_resident_batch_reused_across_growing_requests_matches_fresh_batches(glyphs):
    """One resident batch serves requests that make each of its workspaces grow and its class plan be rebuilt: 16x16 first (small candidate buffer and
    combiner scratch), then 48x48 (nine times the candidate records and work items), MTSDF (four channels: another contour limit, so other class
    lists, and more scratch per contour), SDF without overlap support (no classes at all), MSDF twice in a row (the class plan of the MTSDF call
    must not serve it; if the global-scratch class runs persistent, the second call draws from the other set of work-queue counters) and 16x16
    again (every buffer now larger than it needs).  Each result must equal, bit for bit, what a fresh batch computes for the same request.
    The 1 500 glyphs fork the distance pass into its classes (asserted: LDS class and global-scratch class both launched).  Route counters: at
    48x48 the global-scratch class (77 glyphs at the msdf contour limit of 5: 2 772 work items against a share grid of 763 workgroups) fires
    dist_global_persistent, so the two consecutive MSDF calls alternate the work-queue sets (asserted: that counter rises by 2 over the pair);
    at 16x16 its 308 items stay below the share grid and fire dist_global_direct."""
    sub, xfs, want = glyphs
    small = np.array(xfs, np.float64, copy=True)
    small[:, :2] /= 3                                                         # the 48x48 frames at a third of the scale: 16x16
    no_overlap = M.GeneratorConfig(overlap_support=False)
    requests = [(M.MODE_MSDF, 16, small, None), (M.MODE_MSDF, 48, xfs, None), (M.MODE_MTSDF, 48, xfs, None), (M.MODE_SDF, 48, xfs, no_overlap),
                (M.MODE_MSDF, 48, xfs, None), (M.MODE_MSDF, 48, xfs, None), (M.MODE_MSDF, 16, small, None)]
    fresh = {}
    for mode, size, frames, config in requests:
        if (mode, size) not in fresh:
            fresh[mode, size] = M.GlyphBatch(sub).generate(mode, size, size, frames, config=config).cpu().numpy()
    assert (bits(fresh[M.MODE_MSDF, 48]) == bits(want)).all()
    gb = M.GlyphBatch(sub)
    M.route_counts(reset=True)
    for k, (mode, size, frames, config) in enumerate(requests):
        if k == 4:
            before_pair = M.route_counts()["dist_global_persistent"]
        got = gb.generate(mode, size, size, frames, config=config).cpu().numpy()
        assert (bits(got) == bits(fresh[mode, size])).all(), "request %d (mode %d, %dx%d)" % (k, mode, size, size)
        if k == 1:                                                            # the first 48x48 call forked its classes: this is not the small-launch path
            routes = M.route_counts()
            print("routes after the first 48x48 call:", {name: n for name, n in routes.items() if n})
            assert routes["dist_lds_quad"]+routes["dist_lds_single"] > 0 and routes["dist_global_direct"]+routes["dist_global_persistent"] > 0, routes
        if k == 5:                                                            # the two consecutive MSDF calls each drew from a set of work-queue counters
            assert M.route_counts()["dist_global_persistent"]-before_pair >= 2, M.route_counts()
    routes = M.route_counts()
    print("routes of the sequence:", {name: n for name, n in routes.items() if n})
    assert routes["dist_lds_quad"]+routes["dist_lds_single"] >= 4 and routes["dist_global_direct"]+routes["dist_global_persistent"] >= 4, routes


def test_single_shape_calls_of_many_and_one_contour_share_an_arena(glyphs):
    """A single-shape call on the glyph with the most contours, at once followed by a one-contour glyph on the same thread: the second call takes
    the arena the first one returned, and both build their view over it with borrowed work buffers -- whatever the first call's view had to
    allocate of its own has gone with that view."""
    sub, xfs, want = glyphs
    n_c = np.diff(sub.glyph_contour_offsets)
    many, one = int(np.argmax(n_c)), int(np.flatnonzero(n_c == 1)[0])
    assert n_c[many] >= 10
    for _ in range(2):
        for g in (many, one):
            out = np.zeros((48, 48, 3), np.float32)
            M.generate_msdf(out, sub.shape(g), M.SDFTransformation.from_xf(xfs[g]))
            assert (bits(out) == bits(want[g])).all(), "glyph %d (%d contours)" % (g, n_c[g])


def test_sharded_into_one_interleaved_atlas(glyphs):
    """Two "devices" writing rectangles of ONE float atlas whose memory ranges interleave (column-major placement): a device only ever
    writes its own glyphs' rows, whatever the split."""
    sub, xfs, want = glyphs
    n = 64
    part = sub.select(list(range(n)))
    aw = 8*48
    atlas = np.full((8*48+2, aw, 3), -3., np.float32)
    offs = np.array([(((g % 8)*48+1)*aw+(g//8)*48)*3 for g in range(n)], np.int64)     # glyph g at column g // 8, row block g % 8, one spare row above / below
    M.generate_sharded([0, 0, 0], part, M.MODE_MSDF, 48, 48, xfs[:n], out=atlas, out_offsets=offs, row_stride=aw*3)
    for g in range(n):
        y0, x0 = (g % 8)*48+1, (g//8)*48
        assert (bits(atlas[y0:y0+48, x0:x0+48]) == bits(want[g])).all(), g
    assert (atlas[0] == -3.).all() and (atlas[-1] == -3.).all()


def test_trim_returns_the_pooled_memory(glyphs):
    """msdfhip_trim: the pools of the host-pointer entry points grow to the peak concurrency and are otherwise kept; a process that is
    done with a burst hands them back, and the next call simply builds new ones."""
    import torch
    sub, xfs, want = glyphs
    part = sub.select(list(range(512)))
    hb = M.HostBatch(part)
    out = hb.generate_host(M.MODE_MSDF, 48, 48, xfs[:512])
    one = np.zeros((48, 48, 3), np.float32)
    M.generate_msdf(one, sub.shape(3), M.SDFTransformation.from_xf(xfs[3]))
    hb.close()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    assert L.load().msdfhip_trim() == 0
    after = torch.cuda.mem_get_info()[0]
    assert after > before+(8 << 20), "trim returned only %d bytes of device memory" % (after-before)
    hb = M.HostBatch(part)                                                    # the pools rebuild on demand
    again = hb.generate_host(M.MODE_MSDF, 48, 48, xfs[:512])
    hb.close()
    assert (bits(again) == bits(out)).all() and (bits(out) == bits(want[:512])).all()
    M.generate_msdf(one, sub.shape(3), M.SDFTransformation.from_xf(xfs[3]))
    assert (bits(one) == bits(want[3])).all()


def test_front_door_spreads_over_the_devices_of_msdfhip_devices(glyphs):
    """MSDFHIP_DEVICES (VERDICT r2 next #5c): unmodified callers of the single-shape entry points use every listed device, round robin per
    micro-batched group. On this one-GPU box device 0 is listed twice: 12 threads x 40 calls, every tile identical to the batch path."""
    import os
    sub, xfs, want = glyphs
    lib = L.load()
    os.environ["MSDFHIP_DEVICES"] = "0,0"
    lib.msdfhip_reload_tuning()
    try:
        got = (C.c_int*4)()
        assert lib.msdfhip_front_door_devices(got, 4) == 2 and list(got)[:2] == [0, 0]
        errors = []

        def work(k):
            for i in range(40):
                g = (k*40+i) % sub.n_glyphs
                out = np.zeros((48, 48, 3), np.float32)
                M.generate_msdf(out, sub.shape(g), M.SDFTransformation.from_xf(xfs[g]))
                if not (bits(out) == bits(want[g])).all():
                    errors.append(g)
        ts = [threading.Thread(target=work, args=(k,)) for k in range(12)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errors, errors[:8]
    finally:
        os.environ.pop("MSDFHIP_DEVICES", None)
        lib.msdfhip_reload_tuning()
    assert lib.msdfhip_front_door_devices(None, 0) == 0


def test_streamed_generator_matches_the_resident_pipeline(glyphs):
    """msdfhip_generate_stream_csr (host CSR arrays -> chunks flattened / uploaded / digested under the kernels of the chunks before) against the device
    batch: packed float tiles with a stencil, rectangles of an atlas with gaps (host scatter), the 8-bit atlas; several chunk sizes (also one chunk, and
    chunks far smaller than the list so that every staging slot is reused many times); 1 and many host threads cannot be switched inside one process (the
    pool is created once) -- the sanitizer driver covers the thread counts."""
    sub, xfs, want = glyphs
    lib = L.load()
    n = sub.n_glyphs
    st_want = np.zeros((n, 48, 48), np.uint8)
    hb = M.HostBatch(sub)
    ref = hb.generate_host(M.MODE_MSDF, 48, 48, xfs, stencil=st_want)
    hb.close()
    assert (bits(ref) == bits(want)).all()
    try:
        for chunk in (0, 64, 192, 4096):
            lib.msdfhip_set_pipeline_chunk(chunk)
            st = np.zeros((n, 48, 48), np.uint8)
            got = M.generate_stream(sub, M.MODE_MSDF, 48, 48, xfs, stencil=st)
            assert (bits(got) == bits(want)).all(), chunk
            assert (st == st_want).all(), chunk
    finally:
        lib.msdfhip_set_pipeline_chunk(0)
    # rectangles of an atlas with a gutter: the chunks take the staging + host scatter route
    cols, cell = 32, 50
    rows = (n+cols-1)//cols
    atlas = np.full((rows*cell, cols*cell, 3), -5, np.float32)
    offs = np.array([(((g//cols)*cell+1)*cols*cell+(g % cols)*cell+1)*3 for g in range(n)], np.int64)
    M.generate_stream(sub, M.MODE_MSDF, 48, 48, xfs, out=atlas, out_offsets=offs, row_stride=cols*cell*3)
    for g in (0, 1, 31, 32, 777, n-1):
        y, x = (g//cols)*cell+1, (g % cols)*cell+1
        assert (bits(atlas[y:y+48, x:x+48]) == bits(want[g])).all(), g
    assert (atlas[0] == -5).all() and (atlas[:, 0] == -5).all() and (atlas[cell-1] == -5).all()
    # 8-bit atlas, dense row bands
    cols = 50
    rows = (n+cols-1)//cols
    a8 = np.zeros((rows*48, cols*48, 3), np.uint8)
    offs8 = np.array([((g//cols)*48*cols*48+(g % cols)*48)*3 for g in range(n)], np.int64)
    M.generate_stream(sub, M.MODE_MSDF, 48, 48, xfs, atlas=a8, out_offsets=offs8, row_stride=cols*48*3)
    hb = M.HostBatch(sub)
    b8 = np.zeros_like(a8)
    hb.generate_bytes_host(M.MODE_MSDF, 48, 48, xfs, b8, offs8, cols*48*3)
    hb.close()
    assert (a8 == b8).all()
    # other field types + an empty shape in the list + a list of one
    for mode in (M.MODE_SDF, M.MODE_PSDF, M.MODE_MTSDF):
        few = sub.select(list(range(0, n, 37)))
        w2 = M.GlyphBatch(few).generate(mode, 48, 48, xfs[::37]).cpu().numpy()
        assert (bits(M.generate_stream(few, mode, 48, 48, xfs[::37])) == bits(w2)).all(), mode
    one = sub.select([5])
    assert (bits(M.generate_stream(one, M.MODE_MSDF, 48, 48, xfs[5:6])) == bits(want[5:6])).all()


def test_candidate_overflow_in_a_pipeline_chunk_reruns_the_call(glyphs):
    """The chunks of the host-output pipeline do not launch the per-texel overflow pass of the correction (k_ec_slow) any more: k_ec_query mirrors the
    chunk's candidate-overflow count into pinned memory and a call that had one is run again with the pass (msdfhip_pipeline_overflow_reruns). Overlapping
    strokes rendered WITHOUT overlap support under ALWAYS_CHECK_DISTANCE overflow their candidate segments (tests/test_gpu_parity.py:
    test_candidate_segment_overflow_is_handled_per_glyph): mixed into ordinary glyphs, through packed float tiles, the 8-bit atlas and the streamed generator
    -- bytes must equal the device batch (whose correction always launches the pass), through the rerun that launches it in every chunk."""
    from msdfgen_amd import synth
    from msdfgen_amd.shape import autoframe
    sub, xfs, want48 = glyphs
    lib = L.load()
    shapes = [sub.shape(g) for g in range(0, 600, 3)]
    fr = [xfs[g] for g in range(0, 600, 3)]
    for k, at in enumerate((17, 90, 91, 160)):
        s = synth.cjk_like_shape(8801+k)
        shapes.insert(at, s), fr.insert(at, autoframe(s.bounds(), 48, 48, 4))
    mix, mxf = ShapeBatch.from_shapes(shapes), np.stack(fr)
    c = M.MSDFGeneratorConfig(False, M.ErrorCorrectionConfig(M.EC_EDGE_PRIORITY, M.ALWAYS_CHECK_DISTANCE))
    want = M.GlyphBatch(mix).generate(M.MODE_MSDF, 48, 48, mxf, config=c).cpu().numpy()
    n = mix.n_glyphs
    offs8 = np.arange(n, dtype=np.int64)*48*48*3
    want8 = np.zeros((n, 48, 48, 3), np.uint8)
    hb = M.HostBatch(mix)
    try:
        lib.msdfhip_set_pipeline_chunk(64)
        lib.msdfhip_pipeline_overflow_reruns(1)
        got = hb.generate_host(M.MODE_MSDF, 48, 48, mxf, config=c)
        assert (bits(got) == bits(want)).all()
        assert lib.msdfhip_pipeline_overflow_reruns(1) == 1, "the stroke glyphs were meant to overflow their candidate segments"
        hb.generate_bytes_host(M.MODE_MSDF, 48, 48, mxf, want8, offs8, 48*3, config=c)
        assert lib.msdfhip_pipeline_overflow_reruns(1) == 1
        conv = (255-(np.float32(255.5)-np.float32(255)*np.clip(want, np.float32(0), np.float32(1))).astype(np.int32)).astype(np.uint8)   # pixelFloatToByte
        assert (want8 == conv).all()
        st = np.zeros((n, 48, 48), np.uint8)
        got = M.generate_stream(mix, M.MODE_MSDF, 48, 48, mxf, config=c, stencil=st)
        assert (bits(got) == bits(want)).all() and lib.msdfhip_pipeline_overflow_reruns(1) == 1
        a8 = np.zeros_like(want8)
        M.generate_stream(mix, M.MODE_MSDF, 48, 48, mxf, atlas=a8, out_offsets=offs8, row_stride=48*3, config=c)
        assert (a8 == want8).all()
        # ordinary glyphs only: no second run
        lib.msdfhip_pipeline_overflow_reruns(1)
        plain = M.generate_stream(sub.select(list(range(0, 600, 3))), M.MODE_MSDF, 48, 48, np.stack([xfs[g] for g in range(0, 600, 3)]))
        assert lib.msdfhip_pipeline_overflow_reruns(1) == 0 and (bits(plain) == bits(want48[0:600:3])).all()
    finally:
        lib.msdfhip_set_pipeline_chunk(0)
        hb.close()


def test_automatic_chunk_schedules_at_full_tile_size():
    """The output-specific chunk schedules (float tiles: a quarter chunk, half chunks, ...; 8-bit atlas: 3/8 chunk, full chunks, a falling tail -- msdf_capi.hip:
    runPipelineOnce) only engage with AUTOMATIC chunks and at least two of them: 5 000 glyphs at 64x64 (chunks of 2 048), streamed from host arrays and from a
    resident batch, against the device batch. (tools/stream_sizes_check.py runs 3 000 .. 20 000 glyphs at 32 and 64.)"""
    z = load_npz("dejavu8192.npz")
    full = ShapeBatch(z["glyph_contour_offsets"].astype(np.int32), z["contour_offsets"].astype(np.int32), z["points"], z["types"].astype(np.int32),
                      z["colors"].astype(np.int32), np.zeros(len(z["names"]), bool), [str(n) for n in z["names"]])
    n = 5000
    idx = [(7*i) % 8192 for i in range(n)]
    sub, xfs = full.select(idx), z["xf64"][idx]
    L.load().msdfhip_set_pipeline_chunk(0)
    want = M.GlyphBatch(sub).generate(M.MODE_MSDF, 64, 64, xfs).cpu().numpy()
    assert (bits(M.generate_stream(sub, M.MODE_MSDF, 64, 64, xfs)) == bits(want)).all()
    conv = (255-(np.float32(255.5)-np.float32(255)*np.clip(want, np.float32(0), np.float32(1))).astype(np.int32)).astype(np.uint8)
    offs = np.arange(n, dtype=np.int64)*64*64*3
    a8 = np.zeros((n, 64, 64, 3), np.uint8)
    M.generate_stream(sub, M.MODE_MSDF, 64, 64, xfs, atlas=a8, out_offsets=offs, row_stride=64*3)
    assert (a8 == conv).all()
    hb = M.HostBatch(sub)
    try:
        assert (bits(hb.generate_host(M.MODE_MSDF, 64, 64, xfs)) == bits(want)).all()
        b8 = np.zeros_like(a8)
        hb.generate_bytes_host(M.MODE_MSDF, 64, 64, xfs, b8, offs, 64*3)
        assert (b8 == conv).all()
    finally:
        hb.close()
