"""The GPU side of tests/test_gpu_launch_plan.py, run by it as a child process under a time limit: one GlyphBatch.generate call per case on one 64-glyph
mixed-class group at 24x24 msdf, and what the route counters (msdfhip_debug_route_counts) gained over that call.

    python tests/launchplan_gpu_child.py OUT.json

OUT.json: device (msdfgen_amd.device_info()), contours and edges per glyph, routes {case: {route: increase}}."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import fuzzlib  # noqa: E402

SIZE = (24, 24)
# case -> (table of fuzzlib.TUNINGS or None for the defaults, the -scanline flow)
CASES = {"defaults": (None, False), "short_classes": ("short_classes", False), "quad_classes": ("quad_classes", False), "persistent_grid": ("persistent_grid", False),
         "sign_chunked": ("sign_chunked", True)}


def group():
    """64 glyphs of every distance class: one contour, two contours of few edges, CJK-like, 4-11 contours of few edges."""
    rng = np.random.default_rng(64)
    return [fuzzlib._shape(rng, (5, 6, 2, 3)[i % 4], 9000+i) for i in range(64)]


def counts(shapes):
    co = [np.asarray(s.contour_offsets) for s in shapes]
    return [int(len(c)-1) for c in co], [int(c[-1]-c[0]) for c in co]


def main(out_path):
    import msdfgen_amd as M
    from msdfgen_amd.shape import ShapeBatch, autoframe
    M.init(0)
    info = M.device_info()
    assert info["arch"].startswith("gfx950"), info
    shapes = group()
    w, h = SIZE
    xfs = np.stack([autoframe(s.bounds(), w, h, 2.) for s in shapes])
    routes = {}
    for case, (table, scanline) in CASES.items():
        with fuzzlib.tuned(fuzzlib.TUNINGS[table] if table else {}):
            gb = M.GlyphBatch(ShapeBatch.from_shapes(shapes))
            before = M.route_counts()
            gb.generate(M.MODE_MSDF, w, h, xfs, scanline_pass=scanline).cpu()
            after = M.route_counts()
            gb.close()
        routes[case] = {k: after[k]-before[k] for k in after}
    contours, edges = counts(shapes)
    with open(out_path, "w") as f:
        json.dump({"device": info, "contours": contours, "edges": edges, "routes": routes}, f)
    print("ran %d cases" % len(routes))


if __name__ == "__main__":
    main(sys.argv[1])
