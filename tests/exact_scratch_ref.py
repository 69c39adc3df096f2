"""The two test entries of the exact mode's scratch (include/somhip_test.h: som_debug_exact_scratch_sizes, _held) as dicts: the
order of a BLOCK, written once.  Shared by tests/test_exact_scratch_cpu.py and tests/test_gpu_exact_scratch.py."""
import ctypes as C

PASS = ("stride", "pairs", "max_tiles", "too_large", "gmin", "gflags", "rowcnt", "rowarg", "seed", "plist", "fb_list", "tile_tab", "ctr")
LEVEL = ("n_slots", "n_cstages", "n_img_stages", "Cc", "rg", "csq", "cmax2", "Cst", "Cst_plain")
SORTED = ("cap", "order", "Xb_s", "Xl_s", "Xf_s", "xsq_s", "xerr_s", "seed_s", "sU_s", "lastpos_s")
PLAN = ("stride", "tiles", "sk_keys", "sk_keys2", "sk_vals", "sk_tmp", "scout_g", "tq", "need", "need2", "glist", "gcnt", "tlist", "tcnt",
        "tile_counts", "tile_ticket", "items")
GEOMETRY = ("K", "D", "dp", "stage_bytes", "wide", "item_slots", "pass_rows_override", "pairs_hook")
BLOCK = len(PASS) + 1 + 2 * len(LEVEL) + len(SORTED) + len(PLAN)
assert BLOCK == 59


def _block(v):
    v = [int(x) for x in v]
    a, b = len(PASS), len(PASS) + 1
    return {"pass": dict(zip(PASS, v[:a])), "levels": v[a],
            "cen": [dict(zip(LEVEL, v[b:b + 9])), dict(zip(LEVEL, v[b + 9:b + 18]))],
            "sorted": dict(zip(SORTED, v[b + 18:b + 28])), "plan": dict(zip(PLAN, v[b + 28:b + 45]))}


def geometry(K, D, dp, stage_bytes, wide=0, item_slots=2048, pass_rows_override=0, pairs_hook=0):
    return dict(zip(GEOMETRY, (K, D, dp, stage_bytes, wide, item_slots, pass_rows_override, pairs_hook)))


def sizes(g, rows, stride_cap=0):
    """(ladder without its zeros, the block at the ladder's first stride, the block at first_stride(rows, stride_cap))"""
    from xpysom_dask_amd import _lib
    out = (C.c_int64 * (16 + 2 * BLOCK))()
    g8 = (C.c_int64 * 8)(*[int(g[k]) for k in GEOMETRY])
    assert _lib.load().som_debug_exact_scratch_sizes(g8, rows, stride_cap, out) == 0
    v = list(out)
    ladder = v[:16]
    n = ladder.index(0) if 0 in ladder else 16
    assert all(x == 0 for x in ladder[n:])
    return ladder[:n], _block(v[16:16 + BLOCK]), _block(v[16 + BLOCK:])


def held(engine):
    """What the handle's owners hold: a block (sorted: the resident rows' pass) + "sorted1" (the transient rows') + "geometry"
    + "fbX" / "fb_ids"."""
    out = (C.c_int64 * (BLOCK + 20))()
    engine._check(engine._lib.som_debug_exact_scratch_held(engine._h, out))
    v = [int(x) for x in out]
    b = _block(v[:BLOCK])
    b["sorted1"] = dict(zip(SORTED, v[BLOCK:BLOCK + 10]))
    b["geometry"] = dict(zip(GEOMETRY, v[BLOCK + 10:BLOCK + 18]))
    b["fbX"], b["fb_ids"] = v[BLOCK + 18], v[BLOCK + 19]
    return b
