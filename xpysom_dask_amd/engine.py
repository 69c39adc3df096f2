"""Thin object wrapper over the C handle of libsomhip (include/somhip.h).

`HipEngine` is the only thing the host class talks to.  Its method set is the engine
interface the distributed driver (distributed.py) relies on:
    set_weights / get_weights / set_data / epoch_accumulate / accum_tensor / epoch_merge
"""
import ctypes as C

import numpy as np

from . import _lib


class SomHipError(RuntimeError):
    pass


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


MAX_DENSITY_RADII = 8


def check_radii(radii):
    """The radii of a density query as a float32 array of 1 to 8 values, each >= 0 with a square that is finite in float32
    (include/somhip.h, som_unit_density); anything else is a ValueError.  Needs no engine."""
    try:
        r = np.ascontiguousarray(radii, dtype=np.float32).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("radii must be numbers, got %r" % (radii,)) from None
    if not 1 <= len(r) <= MAX_DENSITY_RADII:
        raise ValueError("between 1 and %d radii, got %d" % (MAX_DENSITY_RADII, len(r)))
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (r.astype(np.float64) ** 2).astype(np.float32)
    bad = ~((r >= 0) & np.isfinite(sq))
    if bad.any():
        raise ValueError("a radius must be >= 0 and its square finite in float32, got %r" % (float(r[np.flatnonzero(bad)[0]]),))
    return r


TOPK_MAX = 8


def check_topk(k):
    """The list length of a top-k query as an int between 1 and 8 (include/somhip.h, SOM_TOPK_MAX); anything else is a ValueError.
    Needs no engine."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an integer, got %r" % (k,))
    if not 1 <= k <= TOPK_MAX:
        raise ValueError("k must be between 1 and %d (SOM_TOPK_MAX), got %d" % (TOPK_MAX, k))
    return int(k)


class HipEngine:
    def __init__(self, x, y, input_len, *, distance="euclidean", neighborhood="gaussian",
                 std_coeff=0.5, compact_support=False, precision="exact", device=0, stream=None,
                 topology="rectangular", norm_p=0, norm_p_real=0.0, missing=None):
        if missing not in _lib.SOM_MISSING:
            raise ValueError("missing must be None or 'nan', got %r" % (missing,))
        self._lib = _lib.load()
        self._h = None
        self.K, self.D = int(x) * int(y), int(input_len)
        self.x, self.y = int(x), int(y)
        self.n_rows = 0
        self._keepalive = None
        self._weights_keepalive = None
        cfg = _lib.SomConfig(int(x), int(y), int(input_len), _lib.SOM_DIST[distance],
                             _lib.SOM_NEIGH[neighborhood], int(bool(compact_support)),
                             _lib.SOM_PREC[precision], int(device), float(std_coeff),
                             C.c_void_p(stream) if stream else None, _lib.SOM_TOPO[topology], int(norm_p), float(norm_p_real),
                             _lib.SOM_MISSING[missing])
        h = C.c_void_p()
        if self._lib.som_create(C.byref(cfg), C.byref(h)) != 0:
            raise SomHipError(self._lib.som_last_error(None).decode())
        self._h = h
        self.has_comm = False
        self.monitoring = False
        self.device = int(device)
        self.precision = precision
        self.missing = missing

    # -- plumbing ---------------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise SomHipError(self._lib.som_last_error(self._h).decode())

    def close(self):
        if self._h is not None:
            self._lib.som_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _fp(a):
        return a.ctypes.data_as(C.POINTER(C.c_float))

    @staticmethod
    def _ip(a):
        return a.ctypes.data_as(C.POINTER(C.c_int32))

    # -- codebook / data --------------------------------------------------------------------
    def set_weights(self, w):
        w = _f32(w).reshape(self.K, self.D)
        self._check(self._lib.som_set_weights(self._h, self._fp(w)))

    def get_weights(self):
        w = np.empty((self.K, self.D), dtype=np.float32)
        self._check(self._lib.som_get_weights(self._h, self._fp(w)))
        return w

    def set_data(self, data):
        data = _f32(data)
        if data.ndim != 2 or data.shape[1] != self.D:
            raise ValueError("data must be (n, %d), got %r" % (self.D, data.shape))
        self._check(self._lib.som_set_data(self._h, self._fp(data), data.shape[0]))
        self.n_rows = data.shape[0]
        self._keepalive = None
        self._weights_keepalive = None        # (new rows: the library has dropped the old rows' weights)

    def set_data_device(self, dev_ptr, n_rows, keepalive=None):
        """Rows already resident in HBM (float32 [n][D]); `keepalive` is whatever owns them."""
        self._check(self._lib.som_set_data_device(self._h, C.c_void_p(dev_ptr), int(n_rows)))
        self.n_rows = int(n_rows)
        self._keepalive = keepalive
        self._weights_keepalive = None

    def set_sample_weights(self, w):
        """Per-row weights of the resident rows (a host array of n_rows finite values >= 0); None clears them."""
        if w is None:
            self._check(self._lib.som_set_sample_weights(self._h, None, 0))
        else:
            w = _f32(w)
            if w.shape != (self.n_rows,):
                raise ValueError("sample weights must have one value per resident row")
            self._check(self._lib.som_set_sample_weights(self._h, self._fp(w), w.shape[0]))
        self._weights_keepalive = None

    def set_sample_weights_device(self, dev_ptr, n_rows, keepalive=None):
        """Weights already resident in HBM (float32 [n_rows], borrowed; contents unchecked); `keepalive` is whatever owns them."""
        self._check(self._lib.som_set_sample_weights_device(self._h, C.c_void_p(dev_ptr), int(n_rows)))
        self._weights_keepalive = keepalive

    def sync_producer(self, stream=None):
        """Wait for the producer of device rows: its `__cuda_array_interface__` stream, or (None) the device."""
        self._check(self._lib.som_sync_producer(self._h, C.c_uint64(int(stream or 0)), int(stream is not None)))

    def copy_to_host(self, dev_ptr, shape):
        """float32 device rows of the caller -> a fresh host array."""
        out = np.empty(shape, dtype=np.float32)
        self._check(self._lib.som_copy_to_host(self._h, C.c_void_p(dev_ptr), C.c_uint64(out.nbytes),
                                               out.ctypes.data_as(C.c_void_p)))
        return out

    # -- one epoch --------------------------------------------------------------------------
    def epoch_accumulate(self, sigma, eta, neigh_f64):
        self._check(self._lib.som_epoch_accumulate(self._h, float(sigma), float(eta), int(bool(neigh_f64))))

    def epoch_accumulate_faithful(self, sigma, eta, neigh_f64):
        """epoch_accumulate through the reference's own formulation (g^T x as one big MFMA GEMM): cross-checks."""
        self._check(self._lib.som_epoch_accumulate_faithful(self._h, float(sigma), float(eta), int(bool(neigh_f64))))

    def epoch_accumulate_forced(self, bmu, sigma, eta, neigh_f64):
        bmu = np.ascontiguousarray(bmu, dtype=np.int32)
        if bmu.shape != (self.n_rows,):
            raise ValueError("bmu must have one id per resident row")
        self._check(self._lib.som_epoch_accumulate_forced(self._h, self._ip(bmu), float(sigma), float(eta),
                                                          int(bool(neigh_f64))))

    def epoch_accumulate_begin(self, sigma, eta, neigh_f64):
        """epoch_accumulate up to stage 1 of the transform; `epoch_accumulate_block` finishes the accumulator
        one map-row block at a time (see include/somhip.h)."""
        self._check(self._lib.som_epoch_accumulate_begin(self._h, float(sigma), float(eta), int(bool(neigh_f64))))

    def epoch_block_count(self):
        n = C.c_int32()
        self._check(self._lib.som_epoch_block_count(self._h, C.byref(n)))
        return n.value

    def epoch_accumulate_block(self, block):
        """Stage 2 of map-row block `block`; returns (offset, n_floats) of the now final slice of the accumulator."""
        off, n = C.c_int64(), C.c_int64()
        self._check(self._lib.som_epoch_accumulate_block(self._h, int(block), C.byref(off), C.byref(n)))
        return off.value, n.value

    # -- the collective inside the library (include/somhip.h, som_comm_*) ---------------------------------
    def comm_unique_id(self):
        """128 opaque bytes from RCCL: rank 0 creates them, the host hands them to every rank."""
        import sys
        if "torch" in sys.modules:                    # share torch's copy of RCCL (and so its HIP runtime)
            path = _lib.torch_lib_file("librccl.so")
            if path:
                self._lib.som_comm_load(path.encode())
        buf = C.create_string_buffer(128)
        if self._lib.som_comm_unique_id(buf) != 0:
            raise SomHipError(self._lib.som_last_error(None).decode())
        return buf.raw

    def comm_init(self, world, rank, unique_id):
        import sys
        if "torch" in sys.modules:
            path = _lib.torch_lib_file("librccl.so")
            if path:
                self._lib.som_comm_load(path.encode())
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self._lib.som_comm_init(self._h, int(world), int(rank), buf))
        self.has_comm = True

    def comm_destroy(self):
        self._check(self._lib.som_comm_destroy(self._h))
        self.has_comm = False

    def epoch_allreduce(self):
        self._check(self._lib.som_epoch_allreduce(self._h))

    def epoch_merge(self):
        self._check(self._lib.som_epoch_merge(self._h))

    def epoch(self, sigma, eta, neigh_f64):
        self._check(self._lib.som_epoch(self._h, float(sigma), float(eta), int(bool(neigh_f64))))

    def pinned_empty(self, shape):
        """A float32 array in pinned host memory: chunks streamed from such arrays are copied
        asynchronously and overlap the previous chunk's kernels (use two and alternate)."""
        import weakref
        n = int(np.prod(shape))
        p = C.c_void_p()
        if self._lib.som_pinned_alloc(C.c_uint64(max(1, n) * 4), C.byref(p)) != 0:
            raise SomHipError("som_pinned_alloc failed")
        buf = (C.c_float * max(1, n)).from_address(p.value)
        arr = np.frombuffer(buf, dtype=np.float32, count=n).reshape(shape)
        weakref.finalize(buf, self._lib.som_pinned_free, p)
        return arr

    def stream_epoch_accumulate(self, chunks, sigma, eta, neigh_f64):
        """epoch_accumulate for rows handed over chunk by chunk: an iterable of (n_i, D) arrays, or of (rows, weights)
        pairs with one sample weight per row -- one form or the other for the whole epoch."""
        self._check(self._lib.som_stream_begin(self._h))
        weighted = None
        for chunk in chunks:
            w = None
            if isinstance(chunk, tuple):
                if len(chunk) != 2:
                    raise ValueError("a weighted chunk is a (rows, weights) pair")
                chunk, w = chunk
            if weighted is None:
                weighted = w is not None
            elif weighted != (w is not None):
                raise ValueError("an epoch's chunks are all rows or all (rows, weights) pairs, not a mix")
            chunk = _f32(chunk)
            if chunk.ndim != 2 or chunk.shape[1] != self.D:
                raise ValueError("chunk must be (n, %d), got %r" % (self.D, chunk.shape))
            if w is None:
                self._check(self._lib.som_stream_rows(self._h, self._fp(chunk), chunk.shape[0]))
            else:
                w = _f32(w)
                if w.shape != (chunk.shape[0],):
                    raise ValueError("a chunk's weights must have one value per row, got %r for %d rows" % (w.shape, chunk.shape[0]))
                self._check(self._lib.som_stream_rows_weighted(self._h, self._fp(chunk), self._fp(w), chunk.shape[0]))
        self._check(self._lib.som_stream_end(self._h, float(sigma), float(eta), int(bool(neigh_f64))))
        self.sync()                       # pinned chunks are copied asynchronously: their buffers are free now

    def epoch_fetch(self, want_bmu=True):
        """(num (K,D), den (K,), bmu (n,) or None) of the last accumulate."""
        num = np.empty((self.K, self.D), dtype=np.float32)
        den = np.empty((self.K,), dtype=np.float32)
        bmu = np.empty((self.n_rows,), dtype=np.int32) if want_bmu else None
        self._check(self._lib.som_epoch_fetch(self._h, self._fp(num), self._fp(den),
                                              self._ip(bmu) if want_bmu else None))
        return num, den, bmu

    def epoch_fetch_masked(self, want_bmu=True):
        """(num (K,D), den (K,D), bmu (n,) or None) of the last accumulate of an engine created with missing='nan': a
        denominator per unit and feature."""
        num = np.empty((self.K, self.D), dtype=np.float32)
        den = np.empty((self.K, self.D), dtype=np.float32)
        bmu = np.empty((self.n_rows,), dtype=np.int32) if want_bmu else None
        self._check(self._lib.som_epoch_fetch_masked(self._h, self._fp(num), self._fp(den),
                                                     self._ip(bmu) if want_bmu else None))
        return num, den, bmu

    def accum_device_ptr(self):
        p, n = C.c_void_p(), C.c_int64()
        self._check(self._lib.som_accum_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def stream_ptr(self):
        """The HIP stream the engine launches on (an integer handle, for torch.cuda.ExternalStream)."""
        p = C.c_void_p()
        self._check(self._lib.som_get_stream(self._h, C.byref(p)))
        return int(p.value or 0)

    def accum_tensor(self):
        """The fused [num|den] accumulator as a torch CUDA tensor aliasing the engine's
        HBM buffer (zero copy) -- what the RCCL all-reduce runs on in place."""
        import torch
        ptr, n = self.accum_device_ptr()

        class _Alias:
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False),
                                        "version": 2, "strides": None}
        return torch.as_tensor(_Alias(), device=torch.device("cuda", self.device))

    # -- inference --------------------------------------------------------------------------
    def bmu(self, x, quantization=False):
        x = _f32(x)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError("x must be (n, %d), got %r" % (self.D, x.shape))
        ids = np.empty((x.shape[0],), dtype=np.int32)
        mode = _lib.SOM_BMU_QUANTIZATION if quantization else _lib.SOM_BMU_ACTIVATION
        self._check(self._lib.som_bmu(self._h, self._fp(x), x.shape[0], mode, self._ip(ids)))
        return ids

    def bmu_device(self, dev_ptr, n_rows, quantization=False):
        """BMU ids of float32 rows that already live in HBM (`dev_ptr`: [n_rows][D], borrowed for the call)."""
        ids = np.empty((int(n_rows),), dtype=np.int32)
        mode = _lib.SOM_BMU_QUANTIZATION if quantization else _lib.SOM_BMU_ACTIVATION
        self._check(self._lib.som_bmu_device(self._h, C.c_void_p(dev_ptr), int(n_rows), mode, self._ip(ids)))
        return ids

    def quantization_error_device(self, dev_ptr, n_rows):
        out = C.c_double()
        self._check(self._lib.som_quantization_error_device(self._h, C.c_void_p(dev_ptr), int(n_rows), C.byref(out)))
        return out.value

    def bmu_f64(self, x):
        """BMUs of float64 rows under the float64 arithmetic NumPy applies to them (som_bmu_f64: euclidean only)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError("x must be (n, %d), got %r" % (self.D, x.shape))
        ids = np.empty((x.shape[0],), dtype=np.int32)
        self._check(self._lib.som_bmu_f64(self._h, x.ctypes.data_as(C.POINTER(C.c_double)), x.shape[0], self._ip(ids)))
        return ids

    def bmu_top2(self, x):
        """(best, second-best) raveled ids under the full Euclidean distance."""
        x = _f32(x)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError("x must be (n, %d), got %r" % (self.D, x.shape))
        a = np.empty((x.shape[0],), dtype=np.int32)
        b = np.empty((x.shape[0],), dtype=np.int32)
        self._check(self._lib.som_bmu_top2(self._h, self._fp(x), x.shape[0], self._ip(a), self._ip(b)))
        return a, b

    def bmu_top2_device(self, dev_ptr, n_rows):
        """(best, second-best) raveled ids of float32 rows that already live in HBM (`dev_ptr`: [n_rows][D], borrowed for the call)."""
        a = np.empty((int(n_rows),), dtype=np.int32)
        b = np.empty((int(n_rows),), dtype=np.int32)
        self._check(self._lib.som_bmu_top2_device(self._h, C.c_void_p(dev_ptr), int(n_rows), self._ip(a), self._ip(b)))
        return a, b

    def distance_matrix(self, x, quantization=False):
        """The (n, K) distance matrix (analysis only)."""
        x = _f32(x)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError("x must be (n, %d), got %r" % (self.D, x.shape))
        out = np.empty((x.shape[0], self.K), dtype=np.float32)
        mode = _lib.SOM_BMU_QUANTIZATION if quantization else _lib.SOM_BMU_ACTIVATION
        self._check(self._lib.som_distance_matrix(self._h, self._fp(x), x.shape[0], mode, self._fp(out)))
        return out

    def quantization_error(self, x):
        x = _f32(x)
        out = C.c_double()
        self._check(self._lib.som_quantization_error(self._h, self._fp(x), x.shape[0], C.byref(out)))
        return out.value

    # -- map diagnostics (include/somhip.h, som_bmu_distances / som_unit_stats) --------------
    def _rows_arg(self, x):
        x = _f32(x)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError("x must be (n, %d), got %r" % (self.D, x.shape))
        return x

    def bmu_distances(self, x):
        """(ids int32, dist float32): every row's unit under the full Euclidean distance and its distance to it, the
        per-row terms of quantization_error."""
        x = self._rows_arg(x)
        ids = np.empty((x.shape[0],), dtype=np.int32)
        dist = np.empty((x.shape[0],), dtype=np.float32)
        self._check(self._lib.som_bmu_distances(self._h, self._fp(x), x.shape[0], self._ip(ids), self._fp(dist)))
        return ids, dist

    def bmu_distances_device(self, dev_ptr, n_rows):
        """bmu_distances of float32 rows that already live in HBM (`dev_ptr`: [n_rows][D], borrowed for the call)."""
        ids = np.empty((int(n_rows),), dtype=np.int32)
        dist = np.empty((int(n_rows),), dtype=np.float32)
        self._check(self._lib.som_bmu_distances_device(self._h, C.c_void_p(dev_ptr), int(n_rows), self._ip(ids), self._fp(dist)))
        return ids, dist

    # -- missing values: the completed rows (include/somhip.h, som_impute) -------------------
    def impute(self, x):
        """(out float32 like x, ids int32): every NaN of a row replaced by what the row's unit (the ACTIVATION search's) holds
        for that feature, everything else bit for bit; a new array, x is not written.  Needs missing='nan'."""
        x = self._rows_arg(x)
        out = np.empty_like(x)
        ids = np.empty((x.shape[0],), dtype=np.int32)
        self._check(self._lib.som_impute(self._h, self._fp(x), x.shape[0], self._fp(out), self._ip(ids)))
        return out, ids

    def impute_device(self, dev_ptr, n_rows, out_ptr):
        """impute of float32 rows that already live in HBM (`dev_ptr`: [n_rows][D], borrowed for the call) into the caller's
        `out_ptr` ([n_rows][D] in HBM; the same pointer: in place).  Returns the ids; the fill is complete on return."""
        ids = np.empty((int(n_rows),), dtype=np.int32)
        self._check(self._lib.som_impute_device(self._h, C.c_void_p(dev_ptr), int(n_rows), C.c_void_p(out_ptr), self._ip(ids)))
        return ids

    def _unit_stats_out(self):
        out = (np.empty((self.K,), dtype=np.int64), np.empty((self.K,), dtype=np.float64), np.empty((self.K,), dtype=np.float64),
               np.empty((self.K,), dtype=np.float32))
        d = C.POINTER(C.c_double)
        return out, (out[0].ctypes.data_as(C.POINTER(C.c_int64)), out[1].ctypes.data_as(d), out[2].ctypes.data_as(d), self._fp(out[3]))

    def unit_stats(self, x):
        """(count int64, sum float64, sumsq float64, max float32), K entries each: per unit, the rows it wins and the sum, the
        sum of squares and the maximum of their distances to it.  Deterministic: the same rows give the same bits."""
        x = self._rows_arg(x)
        out, ptrs = self._unit_stats_out()
        self._check(self._lib.som_unit_stats(self._h, self._fp(x), x.shape[0], *ptrs))
        return out

    def unit_stats_device(self, dev_ptr, n_rows):
        """unit_stats of float32 rows that already live in HBM (`dev_ptr`: [n_rows][D], borrowed for the call)."""
        out, ptrs = self._unit_stats_out()
        self._check(self._lib.som_unit_stats_device(self._h, C.c_void_p(dev_ptr), int(n_rows), *ptrs))
        return out

    # -- data density per unit (include/somhip.h, som_unit_density) --------------------------
    def _density_args(self, pivot, radii):
        radii = check_radii(radii)
        if pivot is not None:
            pivot = _f32(pivot)
            if pivot.shape != (self.D,):
                raise ValueError("pivot must have one value per feature, got %r" % (pivot.shape,))
        out = np.empty((len(radii), self.K), dtype=np.int64)
        return out, (self._fp(pivot) if pivot is not None else None, self._fp(radii), len(radii), out.ctypes.data_as(C.POINTER(C.c_int64))), (pivot, radii)

    def unit_density(self, x, pivot, radii):
        """int64 (len(radii), K): per radius and unit, how many rows lie within the radius of the unit's weight vector (inclusive) --
        the P-matrix.  Euclidean and float32 whatever the engine's distance and precision; `pivot` ((D,) or None) is subtracted from
        rows and units before the GEMM-form distance is formed.  1 to 8 radii in one pass; integer counts, the same in every call."""
        x = self._rows_arg(x)
        out, args, _keep = self._density_args(pivot, radii)
        self._check(self._lib.som_unit_density(self._h, self._fp(x), x.shape[0], *args))
        return out

    def unit_density_device(self, dev_ptr, n_rows, pivot, radii):
        """unit_density of float32 rows that already live in HBM (`dev_ptr`: [n_rows][D], borrowed for the call)."""
        out, args, _keep = self._density_args(pivot, radii)
        self._check(self._lib.som_unit_density_device(self._h, C.c_void_p(dev_ptr), int(n_rows), *args))
        return out

    # -- the k nearest units (include/somhip.h, som_bmu_topk / som_unit_rank_counts) --------------
    def _topk_k(self, k):
        k = check_topk(k)
        if k > self.K:
            raise ValueError("k = %d exceeds the map's %d units" % (k, self.K))
        return k

    def _topk_out(self, n, k, score, dist):
        ids = np.empty((n, k), dtype=np.int32)
        sc = np.empty((n, k), dtype=np.float32) if score else None
        ds = np.empty((n, k), dtype=np.float32) if dist else None
        return ids, sc, ds, (self._ip(ids), self._fp(sc) if score else None, self._fp(ds) if dist else None)

    def bmu_topk(self, x, k, *, score=True, dist=True):
        """(ids int32, score float32 or None, dist float32 or None), each (n, k): per row the k units with the smallest float32
        activation score of the engine's distance, ascending, equal scores to the lower id; `score` those scores (bit for bit the
        entries of distance_matrix), `dist` the Euclidean distance of the row to each listed unit.  Only scores below +inf enter; a
        slot nothing fills holds -1 / NaN / NaN.  Always float32 arithmetic; 1 <= k <= 8 and k <= K."""
        x = self._rows_arg(x)
        k = self._topk_k(k)
        ids, sc, ds, ptrs = self._topk_out(x.shape[0], k, score, dist)
        self._check(self._lib.som_bmu_topk(self._h, self._fp(x), x.shape[0], k, *ptrs))
        return ids, sc, ds

    def bmu_topk_device(self, dev_ptr, n_rows, k, *, score=True, dist=True):
        """bmu_topk of float32 rows that already live in HBM (`dev_ptr`: [n_rows][D], borrowed for the call)."""
        k = self._topk_k(k)
        ids, sc, ds, ptrs = self._topk_out(int(n_rows), k, score, dist)
        self._check(self._lib.som_bmu_topk_device(self._h, C.c_void_p(dev_ptr), int(n_rows), k, *ptrs))
        return ids, sc, ds

    def unit_rank_counts(self, x, k):
        """int64 (k, K): counts[j][u] = the rows whose j-th nearest unit (bmu_topk's slot j) is u, counted on the device -- the
        lists are not copied out.  Integer counts, the same in every call; the counts of chunks add."""
        x = self._rows_arg(x)
        k = self._topk_k(k)
        out = np.empty((k, self.K), dtype=np.int64)
        self._check(self._lib.som_unit_rank_counts(self._h, self._fp(x), x.shape[0], k, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def unit_rank_counts_device(self, dev_ptr, n_rows, k):
        """unit_rank_counts of float32 rows that already live in HBM (`dev_ptr`: [n_rows][D], borrowed for the call)."""
        k = self._topk_k(k)
        out = np.empty((k, self.K), dtype=np.int64)
        self._check(self._lib.som_unit_rank_counts_device(self._h, C.c_void_p(dev_ptr), int(n_rows), k, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    # -- label and value maps (include/somhip.h, som_unit_label_counts / som_unit_value_sums) --
    def _check_columns(self, what, n):
        n = int(n)
        if not 1 <= n <= 4096:
            raise ValueError("%s must be between 1 and 4096, got %d" % (what, n))
        return n

    def _value_sums_out(self, n_cols):
        out = (np.empty((self.K, n_cols), dtype=np.int64), np.empty((self.K, n_cols), dtype=np.float64),
               np.empty((self.K, n_cols), dtype=np.float64))
        d = C.POINTER(C.c_double)
        return out, (out[0].ctypes.data_as(C.POINTER(C.c_int64)), out[1].ctypes.data_as(d), out[2].ctypes.data_as(d))

    def label_counts(self, x, labels, n_classes):
        """int64 (K, n_classes): per unit, how many of the rows it wins under the configured distance (the ids of bmu(x)) carry
        each class code of `labels` (one int32 per row); a code outside [0, n_classes) is unlabelled and counted nowhere."""
        x = self._rows_arg(x)
        n_classes = self._check_columns("n_classes", n_classes)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.shape != (x.shape[0],):
            raise ValueError("labels must have one value per row, got %r for %d rows" % (labels.shape, x.shape[0]))
        out = np.empty((self.K, n_classes), dtype=np.int64)
        self._check(self._lib.som_unit_label_counts(self._h, self._fp(x), self._ip(labels), x.shape[0], n_classes,
                                                    out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def label_counts_device(self, dev_ptr, labels_ptr, n_rows, n_classes):
        """label_counts of float32 rows and int32 labels that already live in HBM (`dev_ptr`: [n_rows][D], `labels_ptr`:
        [n_rows]; both borrowed for the call)."""
        n_classes = self._check_columns("n_classes", n_classes)
        out = np.empty((self.K, n_classes), dtype=np.int64)
        self._check(self._lib.som_unit_label_counts_device(self._h, C.c_void_p(dev_ptr), C.c_void_p(labels_ptr), int(n_rows), n_classes,
                                                           out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def value_sums(self, x, values):
        """(count int64, sum float64, sumsq float64), (K, n_cols) each: per unit and column of `values` ((n, n_cols) float32),
        over the rows the unit wins under the configured distance whose value in the column is not NaN.  Deterministic: the
        same rows give the same bits."""
        x = self._rows_arg(x)
        values = _f32(values)
        if values.ndim != 2 or values.shape[0] != x.shape[0]:
            raise ValueError("values must be (%d, n_cols), got %r" % (x.shape[0], values.shape))
        n_cols = self._check_columns("n_cols", values.shape[1])
        out, ptrs = self._value_sums_out(n_cols)
        self._check(self._lib.som_unit_value_sums(self._h, self._fp(x), self._fp(values), x.shape[0], n_cols, *ptrs))
        return out

    def value_sums_device(self, dev_ptr, values_ptr, n_rows, n_cols):
        """value_sums of float32 rows and values that already live in HBM (`dev_ptr`: [n_rows][D], `values_ptr`:
        [n_rows][n_cols]; both borrowed for the call)."""
        n_cols = self._check_columns("n_cols", n_cols)
        out, ptrs = self._value_sums_out(n_cols)
        self._check(self._lib.som_unit_value_sums_device(self._h, C.c_void_p(dev_ptr), C.c_void_p(values_ptr), int(n_rows), n_cols, *ptrs))
        return out

    # -- row moments and the row gather (include/somhip.h, som_row_moments / som_gather_rows_device) --
    MOMENTS_MAX_FEATURES = 2048

    def _moments_out(self, pivot, gram):
        if pivot is not None:
            pivot = _f32(pivot)
            if pivot.shape != (self.D,):
                raise ValueError("pivot must have one value per feature, got %r" % (pivot.shape,))
        out = (C.c_double(), np.empty((self.D,), dtype=np.float64), np.empty((self.D, self.D), dtype=np.float64) if gram else None)
        d = C.POINTER(C.c_double)
        return pivot, out, (self._fp(pivot) if pivot is not None else None, C.byref(out[0]), out[1].ctypes.data_as(d),
                            out[2].ctypes.data_as(d) if gram else None)

    def row_moments(self, x, weights=None, pivot=None, gram=True):
        """(wsum float, s1 float64 (D,), gram float64 (D, D) or None) of host rows about `pivot` (None: 0): sum w, sum w d and
        sum w d d^T with d = x - pivot in float32.  A query: nothing of the engine's rows, weights or plans changes.  Deterministic."""
        x = self._rows_arg(x)
        if weights is not None:
            weights = _f32(weights)
            if weights.shape != (x.shape[0],):
                raise ValueError("weights must have one value per row, got %r for %d rows" % (weights.shape, x.shape[0]))
        pivot, out, ptrs = self._moments_out(pivot, gram)
        self._check(self._lib.som_row_moments(self._h, self._fp(x), self._fp(weights) if weights is not None else None, x.shape[0], *ptrs))
        return out[0].value, out[1], out[2]

    def row_moments_device(self, dev_ptr, n_rows, weights_ptr=None, pivot=None, gram=True):
        """row_moments of float32 rows (and weights, unchecked) that already live in HBM (`dev_ptr`: [n_rows][D], `weights_ptr`:
        [n_rows] or None; both borrowed for the call): the host entry's bits."""
        pivot, out, ptrs = self._moments_out(pivot, gram)
        self._check(self._lib.som_row_moments_device(self._h, C.c_void_p(dev_ptr), C.c_void_p(weights_ptr) if weights_ptr else None,
                                                     int(n_rows), *ptrs))
        return out[0].value, out[1], out[2]

    def gather_rows_device(self, dev_ptr, n_rows, idx):
        """Rows idx[i] of a float32 device block [n_rows][D] as a host array (len(idx), D); an index outside the block is refused."""
        idx = np.ascontiguousarray(idx, dtype=np.int64).ravel()
        out = np.empty((idx.shape[0], self.D), dtype=np.float32)
        self._check(self._lib.som_gather_rows_device(self._h, C.c_void_p(dev_ptr), int(n_rows), idx.ctypes.data_as(C.POINTER(C.c_int64)),
                                                     idx.shape[0], self._fp(out)))
        return out

    # -- training monitor (include/somhip.h, som_monitor / som_epoch_measure_* / som_epoch_metrics) --
    def monitor(self, on=True):
        """Switch the training monitor on (the engine keeps every measured epoch's BMU ids beside the resident rows) or off
        (frees them).  While it is off nothing is launched or allocated for it."""
        self._check(self._lib.som_monitor(self._h, int(bool(on))))
        self.monitoring = bool(on)

    def epoch_measure_rows(self):
        """Queue the row metrics of the resident rows under this epoch's own BMUs: after any epoch_accumulate* form, before
        the next search."""
        self._check(self._lib.som_epoch_measure_rows(self._h))

    def epoch_measure_shift(self):
        """Queue the codebook shift the merge is about to make: the accumulator must be final (after the all-reduce, or the
        last staged block), before epoch_merge."""
        self._check(self._lib.som_epoch_measure_shift(self._h))

    def epoch_metrics(self):
        """The one blocking read-back: a dict of sum_wd, sum_w, shift_sumsq (float), rows, changed (int; -1 = unknown) and
        shift_max (float)."""
        m = _lib.EpochMetrics()
        self._check(self._lib.som_epoch_metrics(self._h, C.byref(m)))
        return {"sum_wd": m.sum_wd, "sum_w": m.sum_w, "shift_sumsq": m.shift_sumsq, "rows": int(m.rows),
                "changed": int(m.changed), "shift_max": float(m.shift_max)}

    def set_verify(self, n_rows):
        """The canary: re-score `n_rows` strided rows of every BMU launch with the float32 kernel (0 = off)."""
        self._check(self._lib.som_set_verify(self._h, int(n_rows)))

    def verify_stats(self):
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_verify_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_corrupt_operands(self, which=3):
        """TEST HOOK of the canary: zero the operand images behind the library's back (1: 16-bit, 2: float32)."""
        self._check(self._lib.som_debug_corrupt_operands(self._h, int(which)))

    def debug_exact_centroids(self, level):
        """Read-only: (centroids (n_slots, D), radii (n_slots,), |c|^2 (n_slots,)) of the exact plan's level 0 (64-unit groups)
        or 1 (16-unit sub-blocks, slot 16 (g >> 2) + 4 (g & 3) + b) as the device holds them; raises where it holds none."""
        n = C.c_int32()
        self._check(self._lib.som_debug_exact_centroids(self._h, int(level), None, None, None, C.byref(n)))
        cen = np.empty((n.value, self.D), dtype=np.float32)
        rad = np.empty((n.value,), dtype=np.float32)
        csq = np.empty((n.value,), dtype=np.float32)
        self._check(self._lib.som_debug_exact_centroids(self._h, int(level), self._fp(cen), self._fp(rad), self._fp(csq), C.byref(n)))
        return cen, rad, csq

    def debug_mfma16(self, a, b, c, f16=True):
        """Measurement hook: d = a (16x32) . b (32x16) + c (16x16) by ONE 16x16x32 MFMA; a, b float16 (or bfloat16 bit
        patterns as uint16 when f16=False), c float32."""
        a = np.ascontiguousarray(a).view(np.uint16).reshape(16, 32)
        b = np.ascontiguousarray(b).view(np.uint16).reshape(32, 16)
        c = np.ascontiguousarray(c, dtype=np.float32).reshape(16, 16)
        d = np.empty((16, 16), dtype=np.float32)
        self._check(self._lib.som_debug_mfma16(self._h, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                               self._fp(c), self._fp(d), int(bool(f16))))
        return d

    def exact_stats(self):
        """precision 'exact': (rows screened, rows sent to the float32 fallback kernel, screen passes) so far."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.som_exact_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def qe_stats(self):
        """precision 'exact': (rows quantization_error searched with the screen, rows of them sent to the float32 SQRT
        kernel) so far."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_debug_qe_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def exact_top2_stats(self):
        """(rows the top-2 calls served, rows of them the float32 top-2 kernel answered) so far."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_exact_top2_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def exact_chain_stats(self):
        """precision 'exact': planned resident epochs so far that took the sorted rows' last-BMU positions from the epoch
        before instead of gathering them again."""
        a = C.c_int64()
        self._check(self._lib.som_debug_exact_chain_stats(self._h, C.byref(a)))
        return a.value

    def exact_select_stats(self):
        """precision 'exact': (screen passes whose listed screen selected the candidates in its own launch, passes that launched
        the select kernel behind their screen, tiles of the former that the last of their parts selected) so far."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.som_debug_exact_select_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def unit_sort_stats(self):
        """(counting sorts, radix sorts) of rows by their unit the engine ran so far: the segment sums of resident rows and
        streamed chunks, the per-unit queries (csrc/unit_sort.hpp holds the rule that chooses)."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_debug_unit_sort_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_radix_sort(self, keys, bits):
        """(sorted keys, their indices): the stable radix sort of csrc/update.hpp on int32 keys of `bits` bits."""
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        ko, vo = np.empty_like(keys), np.empty_like(keys)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.som_debug_radix_sort(self._h, ip(keys), keys.size, int(bits), ip(ko), ip(vo)))
        return ko, vo

    def debug_exact_select2(self, plist, rmin, gcount, thr2):
        """exact_select2_kernel on copies of plist, rmin [groups][stride], gcount [groups], thr2 [rows]: (plist, gcount, kept)."""
        plist = np.array(plist, dtype=np.int32, order="C")
        rmin = np.ascontiguousarray(rmin, dtype=np.uint32)
        gcount = np.array(gcount, dtype=np.int32, order="C")
        thr2 = np.ascontiguousarray(thr2, dtype=np.uint32)
        assert plist.ndim == 2 and rmin.shape == plist.shape and gcount.shape == plist.shape[:1]
        kept = C.c_int32(-1)
        ip, up = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32)))
        self._check(self._lib.som_debug_exact_select2(self._h, ip(plist), up(rmin), plist.shape[1], ip(gcount), up(thr2),
                                                      plist.shape[0], thr2.size, C.byref(kept)))
        return plist, gcount, kept.value

    def debug_exact_tiles(self, gcount, stride, capacity, blocks, table_entries, gstart=None, want_gstart_out=False):
        """exact_tiles_kernel on a grid of `blocks`: (tile table [table_entries][4], pre-filled with -1, {n_tiles, overflow,
        pairs} started as {-1, 0, -1}, gstart_out pre-filled with -1 or None)."""
        gcount = np.ascontiguousarray(gcount, dtype=np.int32)
        gs = None if gstart is None else np.ascontiguousarray(gstart, dtype=np.int32)
        tab = np.full((int(table_entries), 4), -1, dtype=np.int32)
        out3 = np.array([-1, 0, -1], dtype=np.int32)
        gso = np.full(gcount.shape, -1, dtype=np.int32) if want_gstart_out else None
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        self._check(self._lib.som_debug_exact_tiles(self._h, ip(gcount), ip(gs), gcount.size, int(stride), int(capacity), int(blocks),
                                                    int(table_entries), ip(tab), ip(out3), ip(gso)))
        return tab, out3, gso

    def band_tables(self):
        """(bands on, entries [n][2], P1 [nt][Y][Y], P2 [X][nt * X]): the neighbourhood tables of the last build and the nonzero
        column ranges recorded with them, read back from the device (som_debug_band_tables, include/somhip_test.h)."""
        info = (C.c_int32 * 4)()
        self._check(self._lib.som_debug_band_tables(self._h, info, None, None, None))
        nt, n = info[1], info[2]
        ent = np.zeros((n, 2), dtype=np.int32)
        p1 = np.zeros((nt, self.y, self.y), dtype=np.float32)
        p2 = np.zeros((self.x, nt * self.x), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self._lib.som_debug_band_tables(self._h, info, ent.ctypes.data_as(C.POINTER(C.c_int32)), p1.ctypes.data_as(fp),
                                                    p2.ctypes.data_as(fp)))
        return bool(info[0]), ent, p1, p2

    def band_tables_wrap(self):
        """band_tables() of a toroidal engine: entries [n][2 pieces][2], a low and a high range per 32-row tile and segment
        (som_debug_band_tables_wrap, include/somhip_test.h)."""
        info = (C.c_int32 * 4)()
        self._check(self._lib.som_debug_band_tables_wrap(self._h, info, None, None, None))
        nt, n = info[1], info[2]
        ent = np.zeros((n // 2, 2, 2), dtype=np.int32)
        p1 = np.zeros((nt, self.y, self.y), dtype=np.float32)
        p2 = np.zeros((self.x, nt * self.x), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self._lib.som_debug_band_tables_wrap(self._h, info, ent.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         p1.ctypes.data_as(fp), p2.ctypes.data_as(fp)))
        return bool(info[0]), ent, p1, p2

    def exact_plan_stats(self):
        """precision 'exact': (plans of a screen pass that ran both levels and the lists in one launch, plans that ran them as
        launches of their own) so far."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_debug_exact_plan_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def exact_plan_fold_stats(self):
        """precision 'exact': (plans whose kernels folded the row threshold into the extra MFMA step, plans that compared against
        it -- SOM_EXACT_PLAN_FOLD=0) so far."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_debug_exact_plan_fold_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def exact_last_plan(self):
        """precision 'exact': the plan of the last BMU launch as it ran, a dict of the policy's eight decisions."""
        out = (C.c_int32 * 8)()
        self._check(self._lib.som_debug_exact_last_plan(self._h, out))
        return dict(zip(("skip", "resort", "scout", "level2", "estimate", "sample_tiles", "refine", "time_phases"), (bool(v) for v in out)))

    def exact_forecast(self):
        """precision 'exact': what the last BMU launch learned from its samples, a dict -- need (share of the groups a sampled row
        needs; -1: the row sample was not asked), rows (rows sampled), est / est1 (share of their blocks the sample tiles would run
        after both levels / level 1; -1: not asked), n_st, st (sample tiles, their stride in tiles), blocks_run, groups_run (the
        sample's raw counters), level2 (the sample was planned with level 2; -1: not asked), scout_declined (launches of this
        handle so far whose estimate declined the plan), full_total / full_screen (the policy's measured costs of the last
        launch without a plan, ms per row; 0: none yet)."""
        out = (C.c_double * 12)()
        self._check(self._lib.som_debug_exact_forecast(self._h, out))
        d = dict(zip(("need", "rows", "est", "est1", "n_st", "st", "blocks_run", "groups_run", "scout_declined", "level2", "full_total", "full_screen"),
                     (float(v) for v in out)))
        for k in ("rows", "n_st", "st", "blocks_run", "groups_run", "scout_declined", "level2"):
            d[k] = int(d[k])
        return d

    def exact_tile_blocks(self):
        """precision 'exact', up to 128 features: (16-unit blocks on each tile's list, groups level 1 kept per tile, level 2 ran) of
        the last pass of the last BMU launch as its screen walked them; raises where that launch ran without a plan."""
        info = (C.c_int32 * 2)()
        self._check(self._lib.som_debug_exact_tile_blocks(self._h, None, None, 0, info))
        blocks = np.empty((max(int(info[0]), 0),), dtype=np.int32)
        groups = np.empty_like(blocks)
        self._check(self._lib.som_debug_exact_tile_blocks(self._h, self._ip(blocks), self._ip(groups), blocks.size, info))
        return blocks, groups, bool(info[1])

    def exact_skip_stats(self):
        """precision 'exact': (blocks the screens ran, blocks of full scans) so far -- block skipping's executed share."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_exact_skip_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def exact_resident_stats(self):
        """precision 'exact': (epochs run under a plan, of which (re-)sorted the resident rows by their last BMU's patch)."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_exact_resident_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def exact_scout_stats(self):
        """precision 'exact': (BMU launches that ran the scout, launches over transient row sets that ran under a plan)."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_exact_scout_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def exact_refine_stats(self):
        """precision 'exact': (candidate pairs handed to the refinement pass, pairs it left for the float32 re-score)."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.som_exact_refine_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def exact_last_counts(self, n):
        """precision 'exact': candidate groups per row in the last screen pass (first n rows)."""
        out = np.empty((int(n),), dtype=np.int32)
        self._check(self._lib.som_exact_last_counts(self._h, self._ip(out), int(n)))
        return out

    # -- timing -----------------------------------------------------------------------------
    def sync(self):
        self._check(self._lib.som_sync(self._h))

    def profile_enable(self, on=True):
        self._check(self._lib.som_profile_enable(self._h, 2 if on == "bmu" else int(bool(on))))

    def profile_reset(self):
        self._check(self._lib.som_profile_reset(self._h))

    def profile_get(self, kernel):
        ms, n = C.c_double(), C.c_int64()
        self._check(self._lib.som_profile_get(self._h, _lib.SOM_KERNELS[kernel], C.byref(ms), C.byref(n)))
        return ms.value, n.value
