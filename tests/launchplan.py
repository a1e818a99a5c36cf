"""Binding for the launch plans of msdfgen_amd/csrc/msdf_launchplan.hpp through tests/hostemu (emu_plan_*), shared by tests/test_launch_plan_host.py and
tests/test_gpu_launch_plan.py: an MSDFHIP_* table becomes a PlanEnv the way msdf_capi.hip's readTuning reads it, a plan comes back as dicts, and
planned_routes() lists the route counters one batched generate call bumps."""
import ctypes as C

import numpy as np

from msdfgen_amd.lib import ROUTE_NAMES

ENV_FIELDS = ("resLdsBudget", "persistentRounds", "serialClasses", "querySlotCap", "queryLpcContours", "hasQueryLds", "hasQueryPolicy", "qpEdgeCost", "qpMaxEdges",
              "qpMinCount", "qpWideMaxEdges", "qpWideLoad", "qpWideMeanCount", "signCap", "queryStatic", "queryGridSteps", "queryBatch", "shareGridFactor",
              "persistentGrid", "shortRounds", "smallLaunchTiles", "smallMaxEdges", "ldsClassTpw", "ldsLimit", "cus")
GRES_WORKSPACE_CAP = 1 << 30
STREAM_CALLER, STREAM_SIDE0, STREAM_SIDE1 = 0, 1, 2
EC_ROUTES = ("normal", "stage_snapshot", "slow_all", "too_complex")
CHANNELS = {1: 1, 2: 1, 3: 3, 4: 4}
LAUNCH_FIELDS = ("overlap", "gres", "tpw", "lds_bytes", "global_res", "res_bytes", "idx_bytes", "lds_budget", "mapped", "offset", "count", "stream", "share_grid",
                 "route", "blocks", "persistent", "chunk", "gres_bytes", "list_stride", "max_contours")
HEAD_FIELDS = ("too_complex", "n_launches", "concurrent", "ec_ahead", "unculled", "unculled_overlap", "unculled_mapped", "unculled_offset", "unculled_count",
               "unculled_after_join", "class_limit", "n_one", "n_small", "n_huge", "refused_bytes")
EC_FIELDS = ("too_many_texels", "gres", "res_bytes", "slow_lds", "slow_grid", "snapshot_blocks", "route", "slot_cap", "merged_cap", "slot_offset", "wide_slots",
             "lpc_max_contours", "lpc_edge_cost", "lpc_max_edges", "lpc_min_count", "wide_max_edges", "grid_steps", "query_lds", "fast_lds", "lazy_protect",
             "query_blocks", "query_blocks_resident", "query_flags", "query_batch")
SIGN_FIELDS = ("span", "spans_x", "spans", "blocks", "cap", "lds", "whole_rows", "chunked")


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ll(a):
    return a.ctypes.data_as(C.POINTER(C.c_longlong))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def ec_fast_lds_bytes(n):
    """ecFastLdsBytes (msdf_kernels.hpp): 10x10 halo tile of the field, verdict words and item count, the two item queues."""
    return 10*10*n*4+(64+4)*4+(64*24+64*8)*2


def plan_env(emu, table=None, cus=256, lds_limit=160*1024):
    """The PlanEnv of an MSDFHIP_* table (fuzzlib.TUNINGS style; None: the defaults), parsed as readTuning parses the environment."""
    e = np.zeros(len(ENV_FIELDS))
    assert emu.lib.emu_plan_env_defaults(_d(e)) == len(ENV_FIELDS)
    at = {k: i for i, k in enumerate(ENV_FIELDS)}
    plain = {"MSDFHIP_RES_LDS_BUDGET": "resLdsBudget", "MSDFHIP_PERSISTENT_ROUNDS": "persistentRounds", "MSDFHIP_QUERY_STATIC": "queryStatic",
             "MSDFHIP_QUERY_GRID": "queryGridSteps", "MSDFHIP_SHORT_ROUNDS": "shortRounds", "MSDFHIP_PERSISTENT_GRID": "persistentGrid",
             "MSDFHIP_SHARE_GRID": "shareGridFactor", "MSDFHIP_SMALL_LAUNCH_TILES": "smallLaunchTiles"}
    for k, v in (table or {}).items():
        if k in plain:
            e[at[plain[k]]] = float(v)
        elif k == "MSDFHIP_SERIAL_CLASSES":
            e[at["serialClasses"]] = 1
        elif k == "MSDFHIP_QUERY_LDS":
            e[at["hasQueryLds"]] = 1
            for name, x in zip(("querySlotCap", "queryLpcContours"), v.split(",")):
                e[at[name]] = int(x)
        elif k == "MSDFHIP_QUERY_POLICY":
            e[at["hasQueryPolicy"]] = 1
            for name, x in zip(("qpEdgeCost", "qpMaxEdges", "qpMinCount", "qpWideMaxEdges", "qpWideLoad", "qpWideMeanCount"), v.split(",")):
                e[at[name]] = float(x)
        elif k == "MSDFHIP_SIGN_CAP":
            e[at["signCap"]] = max(int(v), 3)
        elif k == "MSDFHIP_QUERY_BATCH":
            e[at["queryBatch"]] = int(v) if int(v) > 0 else 1
        elif k == "MSDFHIP_SMALL_MAX_EDGES":
            e[at["smallMaxEdges"]] = int(v) if int(v) > 0 else 128
        elif k == "MSDFHIP_LDS_CLASS_TPW":
            e[at["ldsClassTpw"]] = 1 if int(v) == 1 else 4
        else:
            raise KeyError("%s is not a knob of the launch plans" % k)
    e[at["ldsLimit"]], e[at["cus"]] = lds_limit, cus
    return e


def env_field(env, name):
    return env[ENV_FIELDS.index(name)]


def overlap_class_limit(emu, env, nch):
    return emu.lib.emu_overlap_class_limit(_d(env), nch)


def launch_shape(emu, env, n, max_c, max_e, w, h, nch, bound_scratch=True):
    r = emu.lib.emu_launch_shape(_d(env), n, max_c, max_e, w, h, nch, int(bound_scratch))
    return {"huge_batch": bool(r & 1), "small_launch": bool(r & 2)}


def class_list_limit(emu, env, n, max_c, max_e, w, h, nch, overlap, ahead=False):
    return emu.lib.emu_class_list_limit(_d(env), n, max_c, max_e, w, h, nch, int(overlap), int(ahead))


def plan_distance_grid(emu, env, blocks, res_bytes, slots, share_grid=0):
    out = np.zeros(3, np.int64)
    emu.lib.emu_plan_distance_grid(_d(env), C.c_longlong(blocks), C.c_longlong(res_bytes), C.c_longlong(slots), C.c_longlong(share_grid), _ll(out))
    return {"persistent": bool(out[0]), "chunk": int(out[1]), "gres_bytes": int(out[2])}


def plan_distance(emu, env, contours, edges, w, h, mode, overlap, serial_batch=False, want_ec_ahead=False):
    """dispatchDistance's two planning steps on a glyph range given by its per-glyph counts. Returns the plan's head as a dict with "launches" (dicts, issue
    order, "route" by name) and "order" (the class list; None if the call builds none)."""
    c, e = np.ascontiguousarray(contours, np.int32), np.ascontiguousarray(edges, np.int32)
    order = np.full(max(len(c), 1), -1, np.int32)
    head, launches = np.zeros(16, np.int64), np.zeros((4, len(LAUNCH_FIELDS)), np.int64)
    emu.lib.emu_plan_distance(_d(env), _i(c), _i(e), len(c), w, h, CHANNELS[mode], int(overlap), int(serial_batch), int(want_ec_ahead), _i(order), _ll(head),
                              _ll(launches))
    p = {k: int(v) for k, v in zip(HEAD_FIELDS, head)}
    p["launches"] = [dict(zip(LAUNCH_FIELDS, (int(v) for v in launches[k]))) for k in range(p["n_launches"])]
    for l in p["launches"]:
        l["route"] = ROUTE_NAMES[l["route"]]
    p["order"] = order[:len(c)] if p["class_limit"] else None
    return p


def plan_correction(emu, env, n, max_c, max_e, w, h, channels, overlap, ec_mode=2, ec_check=1, stage_limit=0, fast_lds=None, resident=0):
    out = np.zeros(len(EC_FIELDS), np.int64)
    emu.lib.emu_plan_correction(_d(env), n, max_c, max_e, w, h, channels, int(overlap), ec_mode, ec_check, stage_limit,
                                C.c_longlong(ec_fast_lds_bytes(channels) if fast_lds is None else fast_lds), C.c_longlong(resident), _ll(out))
    p = {k: int(v) for k, v in zip(EC_FIELDS, out)}
    p["route"] = EC_ROUTES[p["route"]]
    return p


def plan_sign(emu, env, n, max_e, w, h):
    out = np.zeros(len(SIGN_FIELDS), np.int64)
    emu.lib.emu_plan_sign(_d(env), n, max_e, w, h, _ll(out))
    return {k: int(v) for k, v in zip(SIGN_FIELDS, out)}


def planned_routes(emu, env, contours, edges, w, h, mode, overlap, ec_mode=2, ec_check=1, scanline=False):
    """The route counters one GlyphBatch.generate call on these glyphs bumps, as a sorted list of names (a name per bump)."""
    n, max_c, max_e = len(contours), int(max(contours)), int(max(edges))
    d = plan_distance(emu, env, contours, edges, w, h, mode, overlap)
    assert not d["too_complex"]
    routes = [l["route"] for l in d["launches"]]+["dist_unculled"]*d["unculled"]
    if scanline:
        s = plan_sign(emu, env, n, max_e, w, h)
        routes += ["sign_whole_rows" if s["whole_rows"] else "sign_split"]+["sign_chunked"]*s["chunked"]
    if mode >= 3 and ec_mode != 0:
        c = plan_correction(emu, env, n, max_c, max_e, w, h, CHANNELS[mode], overlap, ec_mode, ec_check)
        if c["route"] == "slow_all":
            routes.append("ec_slow_all")
        elif c["route"] == "normal":                                          # (heaviest-first work lists from 256 glyphs: msdf_capi.hip, ensureEcOrder)
            routes += ["ec_query_heaviest" if n >= 256 else "ec_query_batch"]+["ec_wide_slots"]*c["wide_slots"]
    return sorted(routes)
