"""The band arithmetic of a TOROIDAL table (csrc/update.hpp: band_wrap_mid, band_wrap_piece and band_entry_with, band_tile_range,
band_union per piece) against a NumPy model, through the library's test hook som_debug_band_walk_wrap (include/somhip_test.h).
No device needed.

A toroidal table's nonzeros may lie in two runs of a row, at its start and at its end.  Every segment is cut at the multiple of 8
nearest its middle into a low and a high piece with a range each; a workgroup walks the union of the low ranges, then that
of the high ranges.  As in tests/test_transform_bands_cpu.py the walk is right iff (1) every nonzero of a 32-row tile lies inside
the tile's range of its segment AND PIECE, (2) the columns a workgroup stages per piece contain that piece's range of every one
of its tiles, and what it stages from the piece's `hi` on -- as zeros -- and leaves out below `lo` holds no nonzero of the piece,
(3) ranges are whole skipping groups; and here also (4) the low walk ends at or before the cut and the high walk begins at or
after it, so the columns are walked in ascending order and none twice.  Tightness as there: a tile's range is the smallest run
of whole groups around its piece's nonzeros, a workgroup's the smallest run of chunks (lower end) and columns (upper end)."""
import ctypes as C

import numpy as np
import pytest

TILE, GROUP, CHUNK = 32, 8, 32


def mid_of(segw):
    return ((segw // 2 + GROUP // 2) // GROUP) * GROUP


def band_walk_wrap(H, nseg, segw, wg_rows):
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    H = np.ascontiguousarray(H, dtype=np.float32)
    rows = H.shape[0]
    assert H.shape == (rows, nseg * segw)
    nt, nw = -(-rows // TILE), -(-rows // wg_rows)
    tiles = np.full((nt, nseg, 2, 2), -7, dtype=np.int32)
    wgs = np.full((nw, 2, 3), -7, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    rc = lib.som_debug_band_walk_wrap(H.ctypes.data_as(C.POINTER(C.c_float)), rows, nseg, segw, wg_rows,
                                      tiles.ctypes.data_as(ip), wgs.ctypes.data_as(ip))
    assert rc == 0
    return tiles, wgs


def planted(rng, rows, nseg, segw, kind):
    """A random table with zeros planted the ways a toroidal neighbourhood table has them."""
    H = rng.standard_normal((rows, nseg, segw)).astype(np.float32)
    H[H == 0] = 1.0
    i = np.arange(rows)[:, None, None]
    k = np.arange(segw)[None, None, :]
    s = np.arange(nseg)[None, :, None]
    centre = i * segw // rows
    cyc = np.abs(k - centre)
    cyc = np.minimum(cyc, segw - cyc)                      # cyclic distance of column k from the row's centre
    if kind == "cyclic":                                   # a band around the diagonal that wraps, wider per segment
        H[np.broadcast_to(cyc > 2 + 5 * s, H.shape)] = 0.0
    elif kind == "wider_than_the_side":                    # every column nonzero: the two pieces together are the row, once
        pass
    elif kind == "thin":
        H[np.broadcast_to(cyc != 0, H.shape)] = 0.0
    elif kind == "empty":
        H[:] = 0.0
    elif kind == "seam_only":                              # nonzeros in the first and last columns only, some tiles empty
        w = 1 + 3 * s
        H[np.broadcast_to((k >= w) & (k < segw - w), H.shape)] = 0.0
        H[(np.arange(rows) // TILE) % 3 == 1] = 0.0
    elif kind == "negative_zeros":                         # -0.0 is a zero: it must not widen a range
        H[np.broadcast_to(cyc > 3, H.shape)] = -0.0
        H[rng.random(H.shape) < 0.2] = -0.0
    else:
        raise ValueError(kind)
    return H.reshape(rows, nseg * segw)


KINDS = ["cyclic", "wider_than_the_side", "thin", "empty", "seam_only", "negative_zeros"]
SHAPES = [(256, 256), (160, 160), (129, 129), (97, 97), (65, 65), (33, 33), (40, 300)]


@pytest.mark.parametrize("wg_rows", [64, 128])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nseg", [1, 2, 3])
@pytest.mark.parametrize("rows,segw", SHAPES)
def test_both_pieces_contain_every_nonzero_and_are_tight(rows, segw, nseg, kind, wg_rows):
    rng = np.random.default_rng(rows * 131 + nseg * 17 + segw + len(kind))
    H = planted(rng, rows, nseg, segw, kind)
    tiles, wgs = band_walk_wrap(H, nseg, segw, wg_rows)
    H3 = H.reshape(rows, nseg, segw)
    mid = mid_of(segw)
    assert mid % GROUP == 0 and 0 <= mid <= segw and abs(mid - segw / 2) <= GROUP / 2 + 0.5
    span = [(0, mid), (mid, segw)]                          # the pieces' columns
    per_wg = wg_rows // TILE
    for t in range(tiles.shape[0]):
        for s in range(nseg):
            for p, (a, b) in enumerate(span):
                tlo, thi = (int(v) for v in tiles[t, s, p])
                cols = a + np.flatnonzero((H3[t * TILE:(t + 1) * TILE, s, a:b] != 0).any(axis=0))
                assert tlo % GROUP == 0 and thi % GROUP == 0 and 0 <= tlo <= thi
                if cols.size == 0:
                    assert (tlo, thi) == (0, 0)
                    continue
                assert tlo <= cols[0] and cols[-1] < thi                      # (1)
                assert cols[0] - tlo < GROUP and thi - cols[-1] <= GROUP      # no wider than whole groups need
                assert a <= tlo and thi <= -(-b // GROUP) * GROUP             # (4): a range stays on its side of the cut
    for w in range(wgs.shape[0]):
        block = H3[w * wg_rows:(w + 1) * wg_rows]
        walked = []
        for p, (a, b) in enumerate(span):
            lo, hi, chunks = (int(v) for v in wgs[w, p])
            mine = tiles[w * per_wg:(w + 1) * per_wg, :, p].reshape(-1, 2)
            live = mine[mine[:, 1] > 0]
            if live.size == 0:
                assert (lo, hi, chunks) == (0, 0, 0) and not (block[:, :, a:b] != 0).any()
                continue
            align = GROUP if p else CHUNK                  # (the high walk must not begin below the cut: whole groups, not chunks)
            assert lo % align == 0 and chunks == -(-(hi - lo) // CHUNK) and a <= lo < hi <= b
            assert lo <= live[:, 0].min() and live[:, 1].max() <= lo + CHUNK * chunks     # (2)
            assert not (block[:, :, hi:b] != 0).any() and not (block[:, :, a:lo] != 0).any()
            cols = a + np.flatnonzero((block[:, :, a:b] != 0).any(axis=(0, 1)))
            assert cols[0] - lo < align and hi == cols[-1] + 1                             # tight
            walked.append(np.arange(lo, hi))                                              # (columns from hi on are staged as zeros)
        if walked:
            order = np.concatenate(walked)
            assert (np.diff(order) > 0).all()                                             # (4): ascending, no column twice
        if kind == "wider_than_the_side":
            assert np.array_equal(np.concatenate(walked), np.arange(segw))
        if kind == "seam_only" and segw >= 96 and (block != 0).any():
            assert sum(len(x) for x in walked) < segw                                     # the seam costs two short walks, not the row


def test_cut_is_where_the_header_says():
    for segw, mid in [(256, 128), (160, 80), (129, 64), (97, 48), (65, 32), (33, 16), (300, 152), (96, 48), (32, 16), (7, 0), (3, 0), (200, 104)]:
        assert mid_of(segw) == mid
        H = np.zeros((32, segw), dtype=np.float32)
        H[0, :] = 1.0
        tiles, wgs = band_walk_wrap(H, 1, segw, 64)
        lo_piece, hi_piece = tiles[0, 0]
        if mid > 0:
            assert tuple(lo_piece) == (0, mid)
        else:
            assert tuple(lo_piece) == (0, 0)
        if mid < segw:
            assert hi_piece[0] == mid and hi_piece[1] == -(-segw // GROUP) * GROUP
        else:
            assert tuple(hi_piece) == (0, 0)


def test_bad_arguments_are_refused():
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    H = np.ones((4, 4), dtype=np.float32)
    out = np.zeros(32, dtype=np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert lib.som_debug_band_walk_wrap(H.ctypes.data_as(fp), 4, 1, 4, 96, out.ctypes.data_as(ip), out.ctypes.data_as(ip)) != 0
    assert lib.som_debug_band_walk_wrap(None, 4, 1, 4, 128, out.ctypes.data_as(ip), out.ctypes.data_as(ip)) != 0
    assert lib.som_debug_band_walk_wrap(H.ctypes.data_as(fp), 0, 1, 4, 128, out.ctypes.data_as(ip), out.ctypes.data_as(ip)) != 0
