"""msdf_hostplan.hpp -- the integer planning of the host-output pipeline (chunk schedule, rectangle spans and the one-copy decision, the slots' device
layout) and the glyph ranges of the sharded entry point -- compiled with the host compiler (tests/hostemu). No GPU."""
import ctypes as C

import numpy as np
import pytest

from emu import Emu
from msdfgen_amd.lib import GLYPH_DTYPE

W = H = 8
N = 3
CELL = W*N                                                                    # values per tile row
TILE = W*H*N


@pytest.fixture(scope="module")
def emu():
    e = Emu()
    e.lib.emu_glyph_cost.restype = C.c_double
    return e


def schedule(emu, n_glyphs, chunk, float_output):
    out = np.zeros(n_glyphs+8, np.int32)
    n = emu.lib.emu_chunk_schedule(n_glyphs, chunk, int(float_output), out.ctypes.data_as(C.POINTER(C.c_int)), len(out))
    assert 0 < n <= len(out)
    return out[:n].tolist()


def glyphs(rects):
    """rects: (out_offset, row_stride) per glyph."""
    g = np.zeros(len(rects), GLYPH_DTYPE)
    g["out_offset"] = [r[0] for r in rects]
    g["row_stride"] = [r[1] for r in rects]
    return g


def chunk_span(emu, rects):
    g = glyphs(rects)
    lo = C.c_longlong(-1)
    dense = emu.lib.emu_chunk_span(g.ctypes.data_as(C.c_void_p), len(g), W, H, N, C.byref(lo))
    return bool(dense), lo.value


def rect_span(emu, offset, stride, w, h, n):
    g = glyphs([(offset, stride)])
    lohi = (C.c_longlong*2)()
    emu.lib.emu_rect_span(g.ctypes.data_as(C.c_void_p), w, h, n, lohi)
    return lohi[0], lohi[1]


# ---------------------------------------------------------------------------------------------------------------- chunk schedule

def test_chunk_schedule_pieces_are_positive_sum_up_and_fit_a_slot(emu):
    rng = np.random.default_rng(20261)
    cases = [(int(rng.integers(1, 9001)), int(rng.integers(1, 3001)), bool(rng.integers(0, 2))) for _ in range(4000)]
    cases += [(n, c, f) for n in (1, 2, 63, 64, 65, 127, 128, 129) for c in (1, 2, 63, 64, 65, 128) for f in (False, True)]   # around the 64-glyph granule
    for n_glyphs, chunk, float_output in cases:
        pieces = schedule(emu, n_glyphs, chunk, float_output)
        what = (n_glyphs, chunk, float_output, pieces[:8])
        assert min(pieces) > 0, what
        assert sum(pieces) == n_glyphs, what
        assert max(pieces) <= min(chunk, n_glyphs), what


@pytest.mark.parametrize("n_glyphs, chunk, float_output, want", [
    (8192, 2048, False, [768, 2048, 2048, 2048, 768, 512]),
    (8192, 2048, True, [512]+[1024]*7+[512]),
    (450, 171, False, [64, 171, 171, 21, 23]),                                # a chunk that is no multiple of 64: the oversized piece (192) is cut
    (450, 171, True, [171, 171, 108]),
    (4096, 2048, False, [768, 2048, 768, 512]),
    (129, 64, False, [64, 64, 1]),
    (1, 64, True, [1]),
])
def test_chunk_schedule_of_known_calls(emu, n_glyphs, chunk, float_output, want):
    assert schedule(emu, n_glyphs, chunk, float_output) == want


def test_default_chunk_is_96_mb_of_float_tiles_in_multiples_of_64(emu):
    assert emu.lib.emu_default_chunk(C.c_long(64*64*3)) == 2048               # the bench's tiles: 96 MB / 48 KB
    assert emu.lib.emu_default_chunk(C.c_long(64*64*4)) == 1536
    assert emu.lib.emu_default_chunk(C.c_long(48*48*3)) == 3640//64*64
    assert emu.lib.emu_default_chunk(C.c_long(1024*1024*4)) == 64             # never below 64
    assert emu.lib.emu_default_chunk(C.c_long(0)) > 0


# ---------------------------------------------------------------------------------------------------------------- rectangles

def test_rect_span_for_every_sign_of_the_row_stride(emu):
    assert rect_span(emu, 1000, 72, W, H, N) == (1000, 1000+72*7+CELL)
    assert rect_span(emu, 1000, 0, W, H, N) == (1000, 1000+CELL)
    assert rect_span(emu, 1000, -72, W, H, N) == (1000-72*7, 1000+CELL)       # memory row 0 is the LAST in the buffer
    for stride in (72, 0, -72):                                               # one row: the stride does not matter
        assert rect_span(emu, 1000, stride, W, 1, N) == (1000, 1000+CELL)
    assert rect_span(emu, 2**40, 2**31-1, 5, 3, 4) == (2**40, 2**40+2*(2**31-1)+20)   # 64-bit offsets


GRID_PITCH = 3*CELL                                                           # three cells per row, two cell rows
GRID_BASE = 5*H*GRID_PITCH


def grid_cell(row, col, pitch=GRID_PITCH, base=GRID_BASE):
    return (base+row*H*pitch+col*CELL, pitch)


def test_chunks_that_go_back_as_one_copy(emu):
    packed = [(384+g*TILE, CELL) for g in range(5)]
    assert chunk_span(emu, packed) == (True, 384)
    grid = [grid_cell(r, c) for r, c in ((1, 2), (0, 0), (1, 0), (0, 2), (0, 1), (1, 1))]
    assert chunk_span(emu, grid) == (True, GRID_BASE)
    assert chunk_span(emu, [(77, CELL)]) == (True, 77)


def test_chunks_that_do_not_tile_a_range_are_scattered(emu):
    dense = lambda rects: chunk_span(emu, rects)[0]
    # the historic bug: two glyphs on one cell, another cell free -- the same area and the same extent as the exact tiling
    doubled = [grid_cell(r, c) for r, c in ((1, 2), (0, 0), (1, 0), (0, 1), (0, 1), (1, 1))]
    full = [grid_cell(r, c) for r, c in ((1, 2), (0, 0), (1, 0), (0, 1), (0, 2), (1, 1))]
    span = lambda rects: (min(min(o, o+s*(H-1)) for o, s in rects), max(max(o, o+s*(H-1))+CELL for o, s in rects))   # first and last value of the chunk
    assert span(doubled) == span(full) and len(doubled) == len(full)
    assert dense(full) and not dense(doubled)
    # a pitch that is no multiple of the cell width, with rectangles placed so that the extent still equals the chunk's area (5 tiles)
    pitch = 56
    skewed = [(GRID_BASE+o, pitch) for o in (0, CELL, H*pitch, H*pitch+CELL, H*pitch+4*CELL)]
    assert span(skewed)[1]-span(skewed)[0] == len(skewed)*TILE
    assert not dense(skewed)
    # glyph count that is no multiple of the cells per row: a grid short of its last cell, and four rectangles whose extent equals their area
    assert not dense([grid_cell(r, c) for r, c in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1))])
    ragged = [grid_cell(0, c) for c in (0, 1, 2, 10)]
    assert span(ragged)[1]-span(ragged)[0] == len(ragged)*TILE
    assert not dense(ragged)
    # rows stored bottom-up: the extent and the area of packed tiles, but not their layout
    flipped = [(384+g*TILE+(H-1)*CELL, -CELL) for g in range(4)]
    assert span(flipped) == (384, 384+4*TILE)
    assert not dense(flipped)
    # packed tiles with one gap
    assert not dense([(384+g*TILE+(TILE if g == 3 else 0), CELL) for g in range(4)])
    assert not dense([grid_cell(0, 0), grid_cell(0, 1), grid_cell(0, 1)])


# ---------------------------------------------------------------------------------------------------------------- slot layout

@pytest.mark.parametrize("chunk", [1, 171, 2048])
@pytest.mark.parametrize("w, h, n", [(64, 64, 3), (5, 3, 1), (48, 48, 4)])
@pytest.mark.parametrize("stencil", [False, True])
@pytest.mark.parametrize("bytes_output", [False, True])
def test_slot_layout_regions_are_aligned_ordered_and_disjoint(emu, chunk, w, h, n, stencil, bytes_output):
    texels, tile = w*h, w*h*n
    out = (C.c_longlong*5)()
    emu.lib.emu_slot_layout(chunk, C.c_long(tile), C.c_long(texels), int(stencil), int(bytes_output), out)
    glyphs_at, tiles_at, stencil_at, bytes_at, total = list(out)
    assert glyphs_at == 0
    assert all(o % 256 == 0 for o in (glyphs_at, tiles_at, stencil_at, bytes_at))
    assert tiles_at-glyphs_at >= 2*chunk*GLYPH_DTYPE.itemsize                 # descriptors of the generators and of the byte conversion
    assert stencil_at-tiles_at >= chunk*tile*4                                # float tiles
    assert bytes_at-stencil_at >= (chunk*texels if stencil else 0)
    assert total-bytes_at >= (chunk*tile if bytes_output else 0)              # whichever region is last lies inside
    assert total <= 2*chunk*GLYPH_DTYPE.itemsize+chunk*tile*4+chunk*texels+chunk*tile+5*256   # (and nothing is reserved twice)


# ---------------------------------------------------------------------------------------------------------------- shard ranges

def shard(emu, gco, co, parts):
    gco, co = np.ascontiguousarray(gco, np.int32), np.ascontiguousarray(co, np.int32)
    bounds = np.full(parts+1, -7, np.int32)
    emu.lib.emu_shard_ranges(gco.ctypes.data_as(C.POINTER(C.c_int32)), co.ctypes.data_as(C.POINTER(C.c_int32)), len(gco)-1, parts,
                             bounds.ctypes.data_as(C.POINTER(C.c_int)))
    return bounds.tolist()


def csr(contours, edges_per_contour):
    gco = np.concatenate([[0], np.cumsum(contours)])
    co = np.concatenate([[0], np.cumsum(edges_per_contour)])
    return gco, co


@pytest.fixture(scope="module")
def mixed_glyphs(emu):
    rng = np.random.default_rng(20262)
    contours = np.where(rng.random(300) < .1, 0, rng.integers(1, 13, 300))    # some empty glyphs, one to twelve contours
    heavy = rng.random(int(contours.sum())) < .1
    per_contour = np.where(heavy, rng.integers(40, 200, len(heavy)), rng.integers(1, 12, len(heavy)))
    gco, co = csr(contours, per_contour)
    cost = np.array([emu.lib.emu_glyph_cost(int(gco[g+1]-gco[g]), int(co[gco[g+1]]-co[gco[g]])) for g in range(300)])
    return gco, co, cost


@pytest.mark.parametrize("parts", [1, 2, 3, 8])
def test_shard_ranges_cover_the_list_once_in_equal_modelled_cost(emu, mixed_glyphs, parts):
    gco, co, cost = mixed_glyphs
    n = len(cost)
    bounds = shard(emu, gco, co, parts)
    assert bounds[0] == 0 and bounds[parts] == n
    assert all(a <= b for a, b in zip(bounds, bounds[1:]))
    owner = np.zeros(n, np.int32)
    for k in range(parts):
        owner[bounds[k]:bounds[k+1]] += 1
    assert (owner == 1).all()
    for k in range(parts):
        share = cost[bounds[k]:bounds[k+1]].sum()
        assert abs(share-cost.sum()/parts) <= cost.max()*(1+1e-9), (k, share, cost.sum()/parts, cost.max())


def test_shard_ranges_with_more_parts_than_glyphs_and_without_glyphs(emu):
    gco, co = csr([1, 2, 1], [4, 3, 9, 5])
    bounds = shard(emu, gco, co, 8)
    assert bounds[0] == 0 and bounds[-1] == 3 and all(a <= b for a, b in zip(bounds, bounds[1:]))
    assert sorted(g for k in range(8) for g in range(bounds[k], bounds[k+1])) == [0, 1, 2]
    assert bounds[7] == 3                                                     # the list is used up: the last range is empty
    assert shard(emu, [0], [0], 3) == [0, 0, 0, 0]
    assert shard(emu, [0], [0], 1) == [0, 0]
