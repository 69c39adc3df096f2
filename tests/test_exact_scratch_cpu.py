"""The exact mode's scratch rule (csrc/exact_scratch.hpp) without a device, through som_debug_exact_scratch_sizes.  Every literal
is worked by hand from the rule's expressions; the working stands in the comment beside it."""
import ctypes as C

import pytest

from tests import exact_scratch_ref as E

TAIL = 11 + 16            # ints of the counter block behind its 3 * groups: PassCounters (11 ints) + 64 bytes for a whole-line fill


def k16_stage_bytes(D):
    return (4 * ((D + 31) // 32) + 1) * 1024


def test_small_map_ladder_and_the_pass_at_a_refused_stride():
    # K = 1 024: 16 groups.  pass_rows = 2^32 / (4 * 16) = 67 108 864.  9 000 rows -> round_up(9 000, 256) = 9 216
    g = E.geometry(32 * 32, 24, 32, k16_stage_bytes(24))
    ladder, first, at = E.sizes(g, 9000, 2304)
    # 9 216 / 2 = 4 608; / 2 = 2 304; / 2 = 1 152 -> 1 280 (multiples of 256); 640 -> 768, held at the floor of 1 024; then nothing
    assert ladder == [9216, 4608, 2304, 1280, 1024]
    assert first["pass"]["stride"] == 9216 and at["pass"]["stride"] == 2304
    p = at["pass"]
    # pairs = max(64, min(16 / 4, 512)) = 64; max_tiles = 2 304 * 64 / 128 + 16 = 1 168; gmin = 16 * 2 304; gflags = 16 * 2 304 / 64
    assert (p["pairs"], p["max_tiles"], p["gmin"], p["gflags"], p["too_large"]) == (64, 1168, 36864, 576, 0)
    assert p["plist"] == 36864 and p["rowcnt"] == p["rowarg"] == p["seed"] == p["fb_list"] == 2304
    assert p["tile_tab"] == 1168 and p["ctr"] == 3 * 16 + TAIL
    # the cap only ever lowers the first attempt
    assert E.sizes(g, 9000, 20000)[2]["pass"]["stride"] == 9216 and E.sizes(g, 9000, 0)[2]["pass"]["stride"] == 9216
    assert E.sizes(g, 300, 0)[0] == [512]                    # (under the floor already: nothing smaller is tried)


def test_a_million_rows_of_a_256x256_map_are_one_pass():
    # K = 65 536: 1 024 groups.  pass_rows = 2^32 / 4 096 = 1 048 576
    g = E.geometry(256 * 256, 128, 128, k16_stage_bytes(128))
    ladder, first, _ = E.sizes(g, 1 << 20)
    assert ladder[0] == 1 << 20 and ladder[-1] == 1024 and len(ladder) == 11
    p = first["pass"]
    # pairs = max(64, min(1 024 / 4, 512)) = 256; max_tiles = 2^20 * 256 / 128 + 1 024 = 2 098 176; gmin = plist = 1 024 * 2^20
    assert (p["stride"], p["pairs"], p["max_tiles"]) == (1 << 20, 256, 2098176)
    assert p["gmin"] == p["plist"] == 1 << 30 and p["gflags"] == 1 << 24 and p["too_large"] == 0
    assert E.sizes(g, 3 << 20)[1]["pass"]["stride"] == 1 << 20    # more rows: more passes, not larger ones


@pytest.mark.parametrize("override,want", [(1000, 1024), (73728, 73728), (1500, 1024), (2047, 1024), (2048, 2048)])
def test_pass_rows_override(override, want):
    # rows / 1 024 * 1 024, at least 1 024: 1 000 -> 0 -> 1 024 (the floor); 73 728 = 72 * 1 024 kept; 1 500 -> 1 024
    g = E.geometry(128 * 128, 128, 128, k16_stage_bytes(128), pass_rows_override=override)
    assert E.sizes(g, 147000)[1]["pass"]["stride"] == want


def test_too_large_from_two_to_the_31_on_and_the_pairs_hook():
    base = dict(K=256 * 256, D=128, dp=128, stage_bytes=k16_stage_bytes(128))
    # stride 2^20: 2 047 pairs a row are 2^31 - 2^20 entries, 2 048 are 2^31
    assert E.sizes(E.geometry(pairs_hook=2047, **base), 1 << 20)[1]["pass"]["too_large"] == 0
    assert E.sizes(E.geometry(pairs_hook=2048, **base), 1 << 20)[1]["pass"]["too_large"] == 1
    # ... and one workgroup tile of rows fewer with 2 048: (2^20 - 256) * 2 048 = 2^31 - 2^19
    assert E.sizes(E.geometry(pairs_hook=2048, **base), (1 << 20) - 256)[1]["pass"]["too_large"] == 0
    p = E.sizes(E.geometry(pairs_hook=7, **base), 4096)[1]["pass"]
    assert p["pairs"] == 7 and p["max_tiles"] == 4096 * 7 // 128 + 1024       # the hook replaces max(64, min(groups / 4, 512))
    # 512 x 512: 4 096 groups, min(1 024, 512) = 512 pairs a row
    assert E.sizes(E.geometry(512 * 512, 64, 64, k16_stage_bytes(64)), 4096)[1]["pass"]["pairs"] == 512


def test_centroid_levels():
    # beyond 128 features: one level; 64 x 64 = 64 groups; ncs = ceil(64 / 64) = 1 word; image stages of 32 centroids: 2
    sb = 9 * 1024
    _, b, _ = E.sizes(E.geometry(64 * 64, 136, 192, sb, wide=1), 3000)
    assert b["levels"] == 1
    assert b["cen"][0] == dict(n_slots=64, n_cstages=1, n_img_stages=2, Cc=64 * 136, rg=64, csq=64, cmax2=2, Cst=2 * sb, Cst_plain=2 * sb)
    assert all(v == 0 for v in b["cen"][1].values())
    # up to 128 features, K = 33 * 17 = 561: 9 groups (no multiple of 4 or 64); ncs = 1; level 2: 16 * ceil(9 / 4) = 48 slots, 4 stages
    sb = k16_stage_bytes(128)
    _, b, _ = E.sizes(E.geometry(33 * 17, 128, 128, sb), 5000)
    assert b["levels"] == 2
    assert b["cen"][0] == dict(n_slots=9, n_cstages=1, n_img_stages=1, Cc=9 * 128, rg=9, csq=9, cmax2=2, Cst=sb, Cst_plain=sb)
    assert b["cen"][1] == dict(n_slots=48, n_cstages=4, n_img_stages=4, Cc=48 * 128, rg=48, csq=48, cmax2=2, Cst=4 * sb, Cst_plain=0)
    # 100 x 100: 157 groups; ncs = 3; level 2: 16 * 40 = 640 slots, 12 stages.  256 x 256: 1 024 groups, ncs = 16; 4 096 slots, 64 stages
    _, b, _ = E.sizes(E.geometry(100 * 100, 16, 32, k16_stage_bytes(16)), 5000)
    assert [(c["n_slots"], c["n_cstages"], c["n_img_stages"]) for c in b["cen"]] == [(157, 3, 3), (640, 12, 12)]
    _, b, _ = E.sizes(E.geometry(256 * 256, 16, 32, k16_stage_bytes(16)), 5000)
    assert [(c["n_slots"], c["n_cstages"], c["n_img_stages"]) for c in b["cen"]] == [(1024, 16, 16), (4096, 64, 64)]


def test_sorted_pass():
    g = E.geometry(64 * 64, 30, 32, k16_stage_bytes(30))
    s = E.sizes(g, 20000)[1]["sorted"]                        # 20 000 -> 79 tiles of 256 = 20 224
    assert s == dict(cap=20224, order=20224, Xb_s=20224 * 32, Xl_s=20224 * 32, Xf_s=20224 * 30, xsq_s=20224, xerr_s=20224,
                     seed_s=20224, sU_s=20224, lastpos_s=20224)
    assert E.sizes(g, 20224)[1]["sorted"]["cap"] == 20224 and E.sizes(g, 20225)[1]["sorted"]["cap"] == 20480
    assert E.sizes(g, 128 * 256)[1]["sorted"]["cap"] == 32768          # the forecast's sample: 128 tiles


def test_plan_buffers():
    from xpysom_dask_amd import _lib
    # 64 x 64 up to 128 features: 64 groups, one word a tile at level 1, four at level 2; stride 20 224 = 79 tiles
    g = E.geometry(64 * 64, 32, 32, k16_stage_bytes(32), item_slots=2048)
    q = E.sizes(g, 20000)[1]["plan"]
    assert (q["stride"], q["tiles"], q["tq"]) == (20224, 79, 0)
    assert q["sk_keys"] == q["sk_keys2"] == q["sk_vals"] == q["scout_g"] == 20224
    assert (q["need"], q["need2"], q["glist"], q["tlist"]) == (79, 79 * 4, 79 * 64, 79 * 64 * 4)
    assert q["gcnt"] == q["tcnt"] == q["tile_counts"] == q["tile_ticket"] == 79
    assert q["items"] == 5 * 79 + 4 * 2048 + 16
    out6 = (C.c_int64 * 6)()
    assert _lib.load().som_debug_unit_sort_sizes(20224, 4096, 1, 0, out6) == 0
    assert q["sk_tmp"] == out6[2] == 4 * 20224 + 256 * 10 + 256               # ceil(20 224 / 2 048) = 10 blocks
    assert E.sizes(dict(g, item_slots=1024), 20000)[1]["plan"]["items"] == 5 * 79 + 4 * 1024 + 16
    # beyond 128 features: tq beside the keys, no level 2 (an allocation of none is one of one element)
    w = E.sizes(E.geometry(64 * 64, 136, 192, 9 * 1024, wide=1), 3000)[1]["plan"]
    assert (w["stride"], w["tiles"], w["tq"], w["need"], w["need2"]) == (3072, 12, 3072, 12, 1)


def _counts(b):
    skip = ("too_large",)
    out = [v for k, v in b["pass"].items() if k not in skip]
    for part in (b["cen"][0], b["cen"][1], b["sorted"], b["plan"]):
        out += list(part.values())
    return out


@pytest.mark.parametrize("wide", [0, 1])
def test_no_count_decreases_when_rows_or_stride_grow(wide):
    g = E.geometry(96 * 64, 136 if wide else 64, 192 if wide else 64, 9 * 1024, wide=wide)
    last = None
    for rows in (1, 255, 256, 257, 1000, 1024, 1025, 5000, 20000, 65536, 65537, 300000, 1 << 20, 3 << 20):
        now = _counts(E.sizes(g, rows)[1])
        assert last is None or all(a <= b for a, b in zip(last, now)), rows
        last = now
    last = None
    for cap in (256, 512, 1024, 1280, 2304, 4608, 9216, 65536, 1 << 20):
        now = _counts(E.sizes(g, 3 << 20, cap)[2])
        assert last is None or all(a <= b for a, b in zip(last, now)), cap
        last = now


def test_bad_arguments():
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    g8 = (C.c_int64 * 8)(1024, 24, 32, 5120, 0, 2048, 0, 0)
    out = (C.c_int64 * (16 + 2 * E.BLOCK))()
    assert lib.som_debug_exact_scratch_sizes(g8, 9000, 0, out) == 0
    assert lib.som_debug_exact_scratch_sizes(None, 9000, 0, out) != 0
    assert lib.som_debug_exact_scratch_sizes(g8, 9000, 0, None) != 0
    assert lib.som_debug_exact_scratch_sizes(g8, 0, 0, out) != 0
    assert lib.som_debug_exact_scratch_sizes(g8, 9000, -1, out) != 0
    assert lib.som_debug_exact_scratch_sizes((C.c_int64 * 8)(0, 24, 32, 5120, 0, 2048, 0, 0), 9000, 0, out) != 0
