"""Randomized parity sweep of the HIP path against the oracle (test infrastructure: used by tests/test_gpu_parity.py and tests/test_gpu_routes.py with a
bounded shape count and by tools/fuzz_parity.py for long runs): random shapes (lines / quadratics / cubics, holes, many contours, degenerate
pieces), random tile sizes and ranges, both combiners, every error-correction mode, sdf / psdf / msdf / mtsdf.

plan() draws the groups (pure: numpy and the shape synthesizers, no device); run() renders them on the device and compares every value with the oracle."""
import contextlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

DEFAULT_RATIO = 1.11111111111111111
EC_PAIRS = tuple((m, d) for m in range(4) for d in range(3))
FULL_MIN_GLYPHS, FULL_MIN_TILES = 256, 8192       # scale="full": past MSDFHIP_SMALL_LAUNCH_TILES (8 192) and the 256-glyph bound of the heaviest-first correction order

# Named MSDFHIP_* tables that force the launch routes the sizes of a small sweep would not take (tests/test_gpu_routes.py, tools/fuzz_parity.py --tuning).
TUNINGS = {
    "quad_classes": {"MSDFHIP_SMALL_LAUNCH_TILES": "0", "MSDFHIP_SHORT_ROUNDS": "0"},        # classes with four tiles per wavefront; overlap off: the full-size plan
    "short_classes": {"MSDFHIP_SMALL_LAUNCH_TILES": "0"},                                    # classes in their one-tile short forms
    "lds_class_tpw1": {"MSDFHIP_SMALL_LAUNCH_TILES": "0", "MSDFHIP_SHORT_ROUNDS": "0", "MSDFHIP_LDS_CLASS_TPW": "1"},
    "no_lds_class": {"MSDFHIP_SMALL_LAUNCH_TILES": "0", "MSDFHIP_RES_LDS_BUDGET": "0"},      # every multi-contour glyph in the global-scratch class
    "wide_lds_class": {"MSDFHIP_SMALL_LAUNCH_TILES": "0", "MSDFHIP_RES_LDS_BUDGET": "53248", "MSDFHIP_SMALL_MAX_EDGES": "160"},
    "persistent_grid": {"MSDFHIP_SMALL_LAUNCH_TILES": "0", "MSDFHIP_PERSISTENT_ROUNDS": "1", "MSDFHIP_PERSISTENT_GRID": "40"},
    "serial_classes": {"MSDFHIP_SMALL_LAUNCH_TILES": "0", "MSDFHIP_SERIAL_CLASSES": "1"},
    "query_lds": {"MSDFHIP_QUERY_LDS": "16,2"},
    "query_policy": {"MSDFHIP_QUERY_POLICY": "1,128,0,128,0"},
    "query_counter": {"MSDFHIP_QUERY_STATIC": "0", "MSDFHIP_QUERY_GRID": "0"},
    "sign_chunked": {"MSDFHIP_SIGN_CAP": "3"},
}


@contextlib.contextmanager
def tuned(env):
    """Sets the MSDFHIP_* variables of `env` and has the library read them again; restores both on the way out, failure included."""
    import msdfgen_amd as M
    saved = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update({k: str(v) for k, v in env.items()})
        M.load().msdfhip_reload_tuning()
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        M.load().msdfhip_reload_tuning()


def oracle_threads():
    """Threads for the oracle: the CPUs this process may run on (not the whole host's), at most 16."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 8
    return max(1, min(16, n))


def _shape(rng, kind, sd):
    from msdfgen_amd import synth
    if kind == 0:
        return synth.random_shape(sd, n_contours=int(rng.integers(1, 4)), kinds=(1, 2, 3), holes=bool(sd & 1))
    if kind == 1:
        return synth.random_shape(sd, n_contours=int(rng.integers(1, 3)), edges_per_contour=(3, 14), kinds=(3,), wobble=.6)
    if kind == 2:
        return synth.cjk_like_shape(sd)
    if kind == 4:                                                     # heavily overlapping / nested blobs: texels inside several contours at once
        return synth.random_shape(sd, n_contours=int(rng.integers(3, 8)), kinds=(1, 2, 3), spread=.25, holes=bool(sd & 1))
    if kind == 5:                                                     # one contour: the one-contour class
        return synth.random_shape(sd, n_contours=1, edges_per_contour=(3, 24), kinds=(1, 2, 3))
    if kind == 6:                                                     # two contours of few edges: the LDS-scratch class
        return synth.random_shape(sd, n_contours=2, kinds=(1, 2, 3), holes=bool(sd & 1))
    return synth.random_shape(sd, n_contours=int(rng.integers(4, 12)), edges_per_contour=(3, 6), kinds=(1, 2), spread=.9)


MIXED_KIND = -1                                                       # a group whose shapes each draw their own kind
_MIX_FIRST = (5, 6, 2)                                                # a mixed group starts with one glyph of each distance class


def _plan_geometry(n_shapes, seed, geometry, modes):
    """plan(geometry=...): every group draws one outline family of tests/geomcases.py and one bitmap size (the cases' own sizes by their size, or one
    of geomcases.BIG_SIZES for all), jitters every case by lattice-preserving moves (integer translations and dyadic scales undone by the transform,
    contour order, colour channel permutations, reversed contours) and cycles through the error-correction pairs. A generator of its own: the
    default sequence of draws is not touched."""
    import geomcases
    rng = np.random.default_rng([seed, 0x6e0])
    pairs = [EC_PAIRS[k] for k in rng.permutation(len(EC_PAIRS))]
    order = [list(geometry)[k] for k in rng.permutation(len(geometry))]       # the families in turn: a short sweep has them all
    done = index = 0
    while done < n_shapes:
        family = str(order[index % len(order)])
        size = int(rng.integers(0, 1+len(geomcases.BIG_SIZES)))
        w, h = (None, None) if size == 0 else geomcases.BIG_SIZES[size-1]
        cs = geomcases.bit_exact(geomcases.family_cases(family, 0, w, h))
        if size == 0:                                                 # a batch has one bitmap size: the cases of one of the family's own sizes
            sizes = sorted({(c.w, c.h) for c in cs})
            w, h = sizes[int(rng.integers(0, len(sizes)))]
            cs = [c for c in cs if (c.w, c.h) == (w, h)]
        reps = int(rng.integers(1, 4))
        cs = [c for c in cs for _ in range(reps)]
        framed = [geomcases.jitter(c.shape, c.xf, rng) for c in cs]
        ec_mode, ec_dist = pairs[index % len(pairs)]
        yield {"index": index, "n": len(framed), "mode": int(rng.choice(modes or [1, 2, 3, 3, 4])), "w": w, "h": h, "overlap": index % 2 == 0,
               "ec": (ec_mode, ec_dist), "kind": MIXED_KIND, "shapes": [f[0] for f in framed], "xfs": np.stack([f[1] for f in framed]),
               "y_down": bool(rng.integers(0, 2)), "family": family, "min_dev": DEFAULT_RATIO, "min_imp": DEFAULT_RATIO, "scanline": None,
               "names": [c.name for c in cs]}
        done += len(framed)
        index += 1


def plan(n_shapes, seed, framing=None, scale="small", scanline=False, modes=None, geometry=None):
    """Yields the groups of a sweep as dicts (shapes, transforms and the config of one generate call), drawn from `seed` alone.
    scale="small" with the other arguments at their defaults is the sweep's original sequence of random draws: tests pin seeds to it.
    scale="mixed": groups of 40-80 glyphs whose shape kinds are mixed, so that one launch holds every distance class, and which cycle through
                   the 4 x 3 error-correction pairs, both combiners, Y-down bitmaps and non-default ratios.
    scale="full":  the same at throughput size: at least 256 glyphs and more than 8 192 tiles per group (the launches' large routes).
    scanline: every other group runs the -scanline flow (sign pass between distance and correction), the fill rules in turn.
    modes: the field types to draw from (default sdf, psdf, msdf twice, mtsdf).
    geometry: family names of tests/geomcases.py; the groups then come from _plan_geometry() instead (alone: no framing, scale or scanline with it)."""
    if geometry is not None:
        if framing is not None or scale != "small" or scanline:
            raise ValueError("geometry families go alone")
        yield from _plan_geometry(n_shapes, seed, geometry, modes)
        return
    import xformcases
    from msdfgen_amd.shape import autoframe
    if framing is not None and scale != "small":
        raise ValueError("framing families go with scale='small' only")
    if scale not in ("small", "mixed", "full"):
        raise ValueError("scale must be small, mixed or full")
    rng = np.random.default_rng(seed)
    done = index = scans = 0
    legacy = scale == "small"
    pairs = [EC_PAIRS[k] for k in rng.permutation(len(EC_PAIRS))] if not legacy else None
    while done < n_shapes:
        scan_rule = None
        if scanline and index % 2 == 1:
            scan_rule, scans = scans % 4, scans+1
        if legacy:
            n = int(min(n_shapes-done, rng.integers(20, 80)))
            mode = int(rng.choice(modes or [1, 2, 3, 3, 4]))
            w, h = int(rng.integers(8, 72)), int(rng.integers(8, 72))
            overlap = bool(rng.integers(0, 2))
            ec_mode, ec_dist = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        else:
            mode = int(rng.choice(modes or [1, 2, 3, 3, 4]))
            if scale == "mixed":
                n = int(rng.integers(40, 81))
                w, h = int(rng.integers(24, 57)), int(rng.integers(24, 57))
            elif scan_rule is not None:                               # nGlyphs x tilesY >= 4 096: the sign pass takes whole tile rows
                n = int(rng.integers(456, 521))
                w, h = int(rng.integers(17, 41)), int(rng.integers(65, 73))
            else:
                n = int(rng.integers(FULL_MIN_GLYPHS, 361))
                w, h = int(rng.integers(41, 73)), int(rng.integers(41, 73))
            overlap = index % 2 == 0
            ec_mode, ec_dist = pairs[index % len(pairs)]
        px_range = min(float(rng.choice([2, 4, 8, 1.5])), .45*min(w, h))      # autoframe needs room for the range inside the tile
        kind = int(rng.integers(0, 5)) if legacy else MIXED_KIND
        shapes = []
        for i in range(n):
            sd = int(rng.integers(0, 2**31))
            k = kind if legacy else (_MIX_FIRST[i] if i < len(_MIX_FIRST) else int(rng.choice([0, 1, 2, 3, 4, 5, 6])))
            s = _shape(rng, k, sd)
            s.inverse_y = bool(rng.integers(0, 2))
            shapes.append(s)
        y_down, family, min_dev, min_imp = False, None, DEFAULT_RATIO, DEFAULT_RATIO
        if framing is None:
            xfs = np.stack([autoframe(s.bounds(), w, h, px_range) for s in shapes])
            if rng.random() < .3:                                         # asymmetric range (CLI -arange)
                xfs[:, 4] *= .5
            if not legacy:
                y_down = bool(rng.integers(0, 2))
                if rng.random() < .4:
                    min_dev, min_imp = float(rng.choice([1., 1.05, 1.5, 2.5])), float(rng.choice([1., 1.05, 1.3, 2.]))
        else:
            family = str(rng.choice(list(framing)))
            if family == "tiny_bitmaps":
                w, h = xformcases.TINY_SIZES[int(rng.integers(0, len(xformcases.TINY_SIZES)))]
            framed = [xformcases.frame(family, s, w, h, rng, variant=i) for i, s in enumerate(shapes)]
            shapes = [f[0] for f in framed]
            xfs = np.stack([f[1] for f in framed])
            y_down = bool(rng.integers(0, 2))
        yield {"index": index, "n": n, "mode": mode, "w": w, "h": h, "overlap": overlap, "ec": (ec_mode, ec_dist), "kind": kind, "shapes": shapes,
               "xfs": xfs, "y_down": y_down, "family": family, "min_dev": min_dev, "min_imp": min_imp, "scanline": scan_rule}
        done += n
        index += 1


def _delta(after, before):
    return {k: after[k]-before[k] for k in after}


def run(n_shapes, seed, deadline_s=None, single=False, framing=None, scale="small", scanline=False, tuning=None, modes=None, min_groups=0, stencil=False,
        paths=False, geometry=None, zero_values=(.5,)):
    """Returns a dict: shapes, groups, values_compared, values_differing_bitwise, max_abs_delta, worst_case, seed, routes (route-counter deltas of
    the whole run), group_routes (those of each group's batched call), ...
    single: every shape through its own generate*() call (the literal drop-in: one fused launch per call, msdf_single.hpp) instead of one batch per group.
    framing: family names of tests/xformcases.py; each group then takes one of them (its transforms, Y orientation, and for tiny_bitmaps its bitmap size)
    instead of autoframe. None keeps the autoframed sweep and its exact sequence of random draws.
    geometry: family names of tests/geomcases.py instead (see plan()); NaN and infinity then count as equal only with the same bits.
    scale, scanline, modes: see plan(). tuning: MSDFHIP_* variables set for the run (tuned()).
    min_groups: groups run even past the deadline (a slow box trims a sweep, it does not empty it).
    stencil: the correction's stencil of every batched msdf / mtsdf group with error correction is compared with the oracle's too.
    paths: the same groups also through generate_stream and HostBatch.generate_host (with a stencil): their bytes must equal the batch's.
    zero_values: the sdfZeroValue levels of the sign pass. With more than one, the scanline groups take them in turn: the group's distance mapping is
    moved (same range width) so that distance 0 maps to that level, and the level goes to the product's sign pass and to the oracle's."""
    import time
    import msdfgen_amd as M
    from msdfgen_amd.shape import ShapeBatch
    from oracle.pyoracle import Oracle
    M.init(0)
    orc = Oracle()
    total = differing = 0
    st_total = st_differing = path_total = path_differing = 0
    worst = 0.
    worst_case = None
    groups = 0
    group_routes = []
    pool = ThreadPoolExecutor(max_workers=oracle_threads())
    done = 0
    t0 = time.time()
    seen = set()
    fill_rules = set()
    zeros_used = set()
    scan_groups = 0
    min_glyphs, min_tiles = None, None
    with tuned(tuning or {}):
        routes0 = M.route_counts()
        for grp in plan(n_shapes, seed, framing=framing, scale=scale, scanline=scanline, modes=modes, geometry=geometry):
            if deadline_s is not None and time.time()-t0 >= deadline_s and groups >= min_groups:
                break
            n, mode, w, h, overlap, kind = grp["n"], grp["mode"], grp["w"], grp["h"], grp["overlap"], grp["kind"]
            (ec_mode, ec_dist), shapes, xfs, y_down, family, rule = grp["ec"], grp["shapes"], grp["xfs"], grp["y_down"], grp["family"], grp["scanline"]
            min_dev, min_imp = grp["min_dev"], grp["min_imp"]
            zero = float(zero_values[0])
            if rule is not None and len(zero_values) > 1:
                zero = float(zero_values[scan_groups % len(zero_values)])
                scan_groups += 1
                xfs = np.array(xfs, np.float64)
                width = xfs[:, 5]-xfs[:, 4]                               # DistanceMapping: (d-lower)/(upper-lower); 0 -> zero with lower = -zero*width
                xfs[:, 4] = -zero*width
                xfs[:, 5] = xfs[:, 4]+width
            batch = ShapeBatch.from_shapes(shapes)
            cfg = M.MSDFGeneratorConfig(overlap, M.ErrorCorrectionConfig(ec_mode, ec_dist, min_dev, min_imp)) if mode >= 3 else M.GeneratorConfig(overlap)
            y = M.Y_DOWNWARD if y_down else M.Y_UPWARD
            want_st = stencil and not single and mode >= 3 and ec_mode != 0
            st = None
            if single:
                fn = {1: M.generate_sdf, 2: M.generate_psdf, 3: M.generate_msdf, 4: M.generate_mtsdf}[mode]
                got = np.stack([fn(np.zeros((h, w, M.CHANNELS[mode]), np.float32), shapes[g], M.SDFTransformation.from_xf(xfs[g]), cfg, y) for g in range(n)])
            else:
                import torch
                gb = M.GlyphBatch(batch)
                dst = torch.full((n, h, w), 77, dtype=torch.uint8, device="cuda") if want_st else None
                before = M.route_counts()
                out = gb.generate(mode, w, h, xfs, config=cfg, y_orientation=y, stencil=dst, scanline_pass=rule is not None,
                                  fill_rule=rule if rule is not None else 0, sdf_zero_value=zero)
                group_routes.append(_delta(M.route_counts(), before))
                got = out.cpu().numpy()
                st = dst.cpu().numpy() if want_st else None
                gb.close()
                min_glyphs = n if min_glyphs is None else min(min_glyphs, n)
                tiles = n*((w+7)//8)*((h+7)//8)
                min_tiles = tiles if min_tiles is None else min(min_tiles, tiles)
            if paths and not single and rule is None:
                hst = np.full((n, h, w), 77, np.uint8)
                sst = np.full((n, h, w), 77, np.uint8)
                hb = M.HostBatch(batch)
                hgot = hb.generate_host(mode, w, h, xfs, config=cfg, stencil=hst, y_orientation=y)
                hb.close()
                sgot = M.generate_stream(batch, mode, w, h, xfs, config=cfg, stencil=sst, y_orientation=y)
                for a in (hgot, sgot):
                    path_total += a.size
                    path_differing += int((a.view(np.uint32) != got.view(np.uint32)).sum())
                if want_st:
                    for a in (hst, sst):
                        path_total += a.size
                        path_differing += int((a != st).sum())

            def want(g):
                sb = np.zeros((h, w), np.uint8) if want_st else None
                s = shapes[g]
                if rule is None:
                    f = orc.generate(s, mode, w, h, xfs[g], overlap=overlap, ec_mode=ec_mode, ec_dist=ec_dist, min_dev=min_dev, min_imp=min_imp, y_down=y_down,
                                     stencil=sb)
                else:
                    f = orc.generate(s, mode, w, h, xfs[g], overlap=overlap, ec_mode=0, y_down=y_down)
                    f = orc.sign_correction(s, f, xfs[g], zero, rule, y_down=y_down)
                    if mode >= 3 and ec_mode != 0:
                        f = orc.error_correction(s, f, xfs[g], overlap=overlap, ec_mode=ec_mode, ec_dist=ec_dist, min_dev=min_dev, min_imp=min_imp, y_down=y_down,
                                                 stencil=sb)
                return f, sb
            res = list(pool.map(want, range(n)))
            want_f = np.stack([r[0] for r in res])
            bad = got.view(np.uint32) != want_f.view(np.uint32)
            if geometry is None:
                bad &= ~(np.isnan(got) & np.isnan(want_f))
            total += got.size
            differing += int(bad.sum())
            if want_st:
                want_s = np.stack([r[1] for r in res])
                st_total += st.size
                st_differing += int((st != want_s).sum())
            if bad.any():
                d = np.abs(got.astype(np.float64)-want_f.astype(np.float64))
                d[~bad] = 0
                if geometry is not None:
                    d[np.isnan(d)] = np.inf                           # differing bits where a side is not finite: no smaller than any delta
                m = float(np.nanmax(d))
                if m > worst:
                    worst = m
                    g = int(np.argwhere(bad)[0][0])
                    worst_case = {"mode": mode, "size": [w, h], "overlap": overlap, "ec": [ec_mode, ec_dist], "kind": kind, "glyph_edges": int(shapes[g].n_edges)}
                    if family is not None:
                        worst_case.update(framing=family, y_down=y_down)
                    if scale != "small" or rule is not None:
                        worst_case.update(glyphs=n, glyph=g, y_down=y_down, ratios=[min_dev, min_imp], scanline=rule, tuning=tuning)
            if rule is not None:
                fill_rules.add(rule)
                zeros_used.add(zero)
            seen.add((mode, overlap, ec_mode if mode >= 3 else -1, ec_dist if mode >= 3 else -1, kind, family))
            done += n
            groups += 1
        routes = _delta(M.route_counts(), routes0)
    pool.shutdown()
    return {"shapes": done, "groups": groups, "values_compared": total, "values_differing_bitwise": differing, "max_abs_delta": worst,
            "worst_case": worst_case, "seed": seed, "single_calls": bool(single), "distinct_mode_combiner_ec_kind": len(seen), "seconds": round(time.time()-t0, 1),
            "framings": sorted({k[-1] for k in seen if k[-1] is not None}), "scale": scale, "tuning": tuning or {}, "routes": routes,
            "group_routes": group_routes, "stencil_values_compared": st_total, "stencil_values_differing": st_differing,
            "path_values_compared": path_total, "path_values_differing": path_differing, "fill_rules": sorted(fill_rules), "zero_values": sorted(zeros_used),
            "min_glyphs_per_group": min_glyphs, "min_tiles_per_group": min_tiles}
