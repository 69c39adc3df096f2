"""The transform's band arithmetic (csrc/update.hpp: band_entry_with, band_tile_range, band_union) against a NumPy model, through
the library's test hook som_debug_band_walk (include/somhip_test.h): the host side of the __host__ __device__ functions the
GEMM kernels call.  No device needed.

The transform skips what a range leaves out, so it is right iff (1) every nonzero of a 32-row tile lies inside the tile's range
of its segment, (2) the columns a workgroup stages contain the range of every one of its tiles in every segment, and what it
stages from `hi` on -- as zeros -- holds no nonzero, (3) a tile's range is made of whole skipping groups, which a chunk holds a
whole number of.  How tight the ranges are is checked too: a tile's range is the smallest run of whole groups around its
nonzeros, a workgroup's the smallest run of chunks (the lower end) and columns (the upper end) around its tiles'."""
import ctypes as C

import numpy as np
import pytest

TILE, GROUP, CHUNK = 32, 8, 32


def band_walk(H, nseg, segw, wg_rows):
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    H = np.ascontiguousarray(H, dtype=np.float32)
    rows = H.shape[0]
    assert H.shape == (rows, nseg * segw)
    nt, nw = -(-rows // TILE), -(-rows // wg_rows)
    tiles = np.full((nt, nseg, 2), -7, dtype=np.int32)
    wgs = np.full((nw, 3), -7, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    rc = lib.som_debug_band_walk(H.ctypes.data_as(C.POINTER(C.c_float)), rows, nseg, segw, wg_rows, tiles.ctypes.data_as(ip),
                                 wgs.ctypes.data_as(ip))
    assert rc == 0
    return tiles, wgs


def planted(rng, rows, nseg, segw, kind):
    """A random table with zeros planted the ways the neighbourhood tables have them."""
    H = rng.standard_normal((rows, nseg, segw)).astype(np.float32)
    i = np.arange(rows)[:, None, None]
    k = np.arange(segw)[None, None, :]
    s = np.arange(nseg)[None, :, None]
    if kind == "dense":
        pass
    elif kind == "band":                                   # a diagonal band, a different half-width per segment
        H[np.broadcast_to(np.abs(i * segw // rows - k) > 2 + 5 * s, H.shape)] = 0.0
    elif kind == "thin":                                   # narrower than one group
        H[np.broadcast_to(i * segw // rows != k, H.shape)] = 0.0
    elif kind == "blocks":                                 # whole tiles and whole segments empty, single nonzeros elsewhere
        H[:] = 0.0
        for _ in range(max(1, rows // 16)):
            H[rng.integers(rows), rng.integers(nseg), rng.integers(segw)] = -1.0
        H[(np.arange(rows) // TILE) % 3 == 1] = 0.0
    elif kind == "sparse":                                 # random zeros, random survivors anywhere (negative zeros too)
        H[rng.random(H.shape) < 0.97] = 0.0
        H[rng.random(H.shape) < 0.01] = -0.0
    elif kind == "empty":
        H[:] = 0.0
    return H.reshape(rows, nseg * segw)


@pytest.mark.parametrize("wg_rows", [64, 128])
@pytest.mark.parametrize("kind", ["dense", "band", "thin", "blocks", "sparse", "empty"])
@pytest.mark.parametrize("rows,nseg,segw", [(256, 1, 256), (160, 1, 160), (129, 3, 129), (97, 2, 97), (65, 6, 65), (33, 1, 33),
                                             (7, 2, 7), (200, 1, 31), (512, 1, 512), (40, 4, 300)])
def test_ranges_contain_every_nonzero_and_are_tight(rows, nseg, segw, kind, wg_rows):
    rng = np.random.default_rng(rows * 131 + nseg * 17 + segw + len(kind))
    H = planted(rng, rows, nseg, segw, kind)
    tiles, wgs = band_walk(H, nseg, segw, wg_rows)
    H3 = H.reshape(rows, nseg, segw)
    per_wg = wg_rows // TILE
    for t in range(tiles.shape[0]):
        for s in range(nseg):
            tlo, thi = (int(v) for v in tiles[t, s])
            cols = np.flatnonzero((H3[t * TILE:(t + 1) * TILE, s, :] != 0).any(axis=0))
            assert tlo % GROUP == 0 and thi % GROUP == 0 and 0 <= tlo <= thi
            if cols.size == 0:
                assert (tlo, thi) == (0, 0)
                continue
            assert tlo <= cols[0] and cols[-1] < thi                      # (1)
            assert cols[0] - tlo < GROUP and thi - cols[-1] <= GROUP      # no wider than whole groups need
    for w in range(wgs.shape[0]):
        lo, hi, chunks = (int(v) for v in wgs[w])
        mine = tiles[w * per_wg:(w + 1) * per_wg].reshape(-1, 2)
        live = mine[mine[:, 1] > 0]
        block = H3[w * wg_rows:(w + 1) * wg_rows]
        if live.size == 0:
            assert (lo, hi, chunks) == (0, 0, 0) and not (block != 0).any()
            continue
        assert lo % CHUNK == 0 and chunks == -(-(hi - lo) // CHUNK) and 0 <= lo < hi <= segw
        assert lo <= live[:, 0].min() and live[:, 1].max() <= lo + CHUNK * chunks      # (2): staged columns hold every tile's range
        assert not (block[:, :, hi:] != 0).any() and not (block[:, :, :lo] != 0).any()  # ... and nothing nonzero is staged as zero
        cols = np.flatnonzero((block != 0).any(axis=(0, 1)))
        assert cols[0] - lo < CHUNK and hi == cols[-1] + 1                               # tight


def test_bad_arguments_are_refused():
    from xpysom_dask_amd import _lib
    lib = _lib.load()
    H = np.ones((4, 4), dtype=np.float32)
    out = np.zeros(16, dtype=np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert lib.som_debug_band_walk(H.ctypes.data_as(fp), 4, 1, 4, 96, out.ctypes.data_as(ip), out.ctypes.data_as(ip)) != 0
    assert lib.som_debug_band_walk(None, 4, 1, 4, 128, out.ctypes.data_as(ip), out.ctypes.data_as(ip)) != 0
    assert lib.som_debug_band_walk(H.ctypes.data_as(fp), 0, 1, 4, 128, out.ctypes.data_as(ip), out.ctypes.data_as(ip)) != 0
