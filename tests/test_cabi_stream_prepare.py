"""The streamed generator over RAW outlines (msdfhip_generate_stream_prepared / _csr_prepared) at the C-ABI surface, without a GPU: both entry points
are exported, and their own argument checks (a NULL preparation config, a colouring strategy outside 0..2, a stencil with 8-bit output) answer
MSDFHIP_ERR_INVALID before anything touches a device -- so the answer is the same with and without one."""
import ctypes as C

import numpy as np

from msdfgen_amd import lib as L

COUNT = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32))
FILL = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8))


class ShapeSource(C.Structure):
    """MsdfHipShapeSource."""
    _fields_ = [("user", C.c_void_p), ("count", COUNT), ("fill", FILL)]


def _triangle():
    gco = np.array([0, 1], np.int32)
    co = np.array([0, 3], np.int32)
    pts = np.zeros((3, 8), np.float64)
    pts[0, :4] = (0, 0, 1, 0)
    pts[1, :4] = (1, 0, 0, 1)
    pts[2, :4] = (0, 1, 0, 0)
    types = np.ones(3, np.uint8)
    glyphs = np.zeros(1, L.GLYPH_DTYPE)
    glyphs["xf"][0] = (8, 8, 0, 0, 1, 0)
    glyphs["row_stride"] = 8*3
    return gco, co, pts, types, glyphs


def test_prepared_stream_entry_points_are_exported():
    lib = L.load()
    for name in ("msdfhip_generate_stream_prepared", "msdfhip_generate_stream_csr_prepared"):
        assert hasattr(lib, name), name
        assert name in L.EXPORTED_SYMBOLS, name
    assert lib.msdfhip_abi_version() == 5


def test_prepared_stream_validates_arguments_before_the_device():
    lib = L.load()
    cfg = L.default_config()
    gco, co, pts, types, glyphs = _triangle()
    out = np.zeros((1, 8, 8, 3), np.float32)
    atlas = np.zeros((1, 8, 8, 3), np.uint8)
    stencil = np.zeros((1, 8, 8), np.uint8)

    def csr(prep, to_atlas=False, st=None):
        return lib.msdfhip_generate_stream_csr_prepared(-1, 3, 8, 8, 1, L.ptr(gco, L._ip), L.ptr(co, L._ip), L.ptr(pts, L._dp), L.ptr(types, L._bp), None,
                                                        glyphs.ctypes.data, None if to_atlas else out.ctypes.data, 0 if to_atlas else out.size,
                                                        atlas.ctypes.data if to_atlas else None, atlas.size if to_atlas else 0,
                                                        st.ctypes.data if st is not None else None, C.byref(cfg), C.byref(prep) if prep is not None else None, None)

    called = []
    count = COUNT(lambda user, g, nc, ne: called.append(g))
    fill = FILL(lambda user, g, base, ends, p, t, c: called.append(g))
    source = ShapeSource(None, count, fill)

    def src(prep, to_atlas=False, st=None):
        return lib.msdfhip_generate_stream_prepared(-1, 3, 8, 8, 1, C.byref(source), glyphs.ctypes.data, None if to_atlas else out.ctypes.data,
                                                    0 if to_atlas else out.size, atlas.ctypes.data if to_atlas else None, atlas.size if to_atlas else 0,
                                                    st.ctypes.data if st is not None else None, C.byref(cfg), C.byref(prep) if prep is not None else None, None)

    for call in (csr, src):
        assert call(None) == L.ERR_INVALID
        assert b"prep" in lib.msdfhip_last_error()
        for coloring in (-1, 3):
            assert call(L.PrepConfig(1, coloring, 3.0, 0)) == L.ERR_INVALID
            assert b"coloring" in lib.msdfhip_last_error()
        assert call(L.PrepConfig(1, 1, 3.0, 0), to_atlas=True, st=stencil) == L.ERR_INVALID
        assert b"stencil" in lib.msdfhip_last_error()
    assert not called, "the shape source was read before the arguments were checked"
    assert not out.any() and not atlas.any() and not stencil.any()
