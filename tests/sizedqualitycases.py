"""Shared by tests/test_sized_quality_host.py and tests/test_gpu_sized_quality.py: the render cases, the oracle's fields of the 43 glyphs of
tests/test_gpu_sized.py, and the plan of the sized error estimate restated from its documented formulas (msdfgen_amd/csrc/msdf_qualityplan.hpp)."""
import numpy as np

PAIRS = ((1, 1), (3, 1), (1, 3), (3, 3), (1, 4), (4, 4))                   # (output channels, field channels): renderSDF's six overloads
MODE_OF_CHANNELS = {1: 1, 3: 3, 4: 4}                                      # the generator mode that gives a field of that many channels
RANGES = ((-1., 1.), (2., -1.), (0., 0.))                                  # a range, an inverted one, the threshold form
THRESHOLDS = (.5, .4)
N_OUT_SIZES = 4


def out_sizes(w, h):
    return ((2*w, 2*h), (w, h), (1, 1), (3*w+1, max(h//2, 1)))


_FIELDS = {}


def fields(oracle, mode):
    """The oracle's w_g x h_g field of every glyph of test_gpu_sized.glyphs() in `mode` (no error correction): computed once, shared, never written to."""
    if mode not in _FIELDS:
        from test_gpu_sized import glyphs
        shapes, sizes, xfs = glyphs()
        out = []
        for s, (w, h), xf in zip(shapes, sizes, xfs):
            f = oracle.generate(s, mode, int(w), int(h), xf, ec_mode=0)
            f.setflags(write=False)
            out.append(f)
        _FIELDS[mode] = out
    return _FIELDS[mode]


def item_prefix(sizes, spr):
    """itemStart[g+1] = itemStart[g] + (w_g > 1 and h_g > 1 ? (h_g-1)*spr : 0)."""
    start = [0]
    for w, h in np.asarray(sizes).reshape(-1, 2).tolist():
        start.append(start[-1]+((h-1)*spr if w > 1 and h > 1 else 0))
    return start


def lane_bytes(max_edges, width):
    """A lane's two lists: 3*max(maxEdges, 1) + 3*W+2 entries of a double and an int."""
    return (3*max(max_edges, 1)+3*width+2)*12


def chunk_lanes(items, per_lane, cap_bytes):
    """Lanes per launch: what the cap holds, at least 64, a multiple of 64, no more than the items rounded up to 64."""
    lanes = max(64, cap_bytes//per_lane//64*64)
    return min(lanes, (items+63)//64*64)
