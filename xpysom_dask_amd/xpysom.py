"""XPySom -- the reference's class surface over the MI355X HIP engine.

Drop-in for ``xpysom_dask.XPySom`` (reference xpysom_dask/xpysom.py:72-892) on its hot path:
``__init__``, ``train``, ``winner``, ``quantization_error`` (+ the thin consumers of those).
The host keeps what the reference keeps on the host -- argument validation and error
strings, the seeded default codebook, the sigma/eta schedules, the epoch loop, result
formatting, pickling -- and hands everything below ``_update``/``_winner``/``_merge_updates``
to libsomhip through ctypes.  There is no ``xp=`` dispatch and no CPU path: without the HIP
library (or a GPU) the compute methods raise.
"""
from collections import Counter, defaultdict, namedtuple
from warnings import warn

import numpy as np

from . import distributed as _dist
from .decays import DECAY_FUNCTIONS

TOPOLOGIES = ("hexagonal", "rectangular", "toroidal")
# name -> implemented in the HIP engine?   (registry order follows xpysom.py:260-283)
NEIGHBORHOODS = {"gaussian": True, "mexican_hat": True, "bubble": True, "triangle": True}
# distances.py:162-170 registry; False = valid reference name the engine does not cover yet
DISTANCES = {"euclidean": True, "euclidean_no_opt": True, "manhattan": True, "manhattan_no_opt": True,
             "cosine": True, "norm_p": True, "norm_p_no_opt": True}
DEFAULT_BATCH_ROWS = 65536


def _device_rows(data):
    """Rows that already live in HBM (the role CuPy arrays play in the reference, xpysom.py:487-510):
    a torch CUDA tensor, or any object with ``__cuda_array_interface__``, as a contiguous float32
    ``(n, input_len)`` block.  Returns ``(pointer, n_rows, n_cols, device_index, owner, stream)`` or ``None``
    for host data; ``stream`` is the producer's stream in ``__cuda_array_interface__`` terms (``None``: the
    producer named none -- the engine then waits for the whole device; ``"done"``: already waited for)."""
    torch = None
    if type(data).__module__.split(".")[0] == "torch":   # (torch is imported only when a tensor is actually passed)
        import torch
    if torch is not None and isinstance(data, torch.Tensor):
        if not data.is_cuda:
            return None
        t = data.detach()
        if t.dim() != 2:
            raise ValueError('data must be 2-dimensional (n_samples, input_len)')
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        torch.cuda.current_stream(t.device).synchronize()      # the engine reads it on its own stream
        return t.data_ptr(), t.shape[0], t.shape[1], t.device.index, t, "done"
    cai = getattr(data, "__cuda_array_interface__", None)
    if cai is not None:
        shape = tuple(cai["shape"])
        if len(shape) != 2 or cai["typestr"] != "<f4" or cai.get("strides") is not None:
            raise ValueError('device data must be a C-contiguous float32 (n_samples, input_len) array')
        return int(cai["data"][0]), shape[0], shape[1], None, data, cai.get("stream")
    return None


def _n_rows(data):
    """Row count of host or device data without touching it."""
    shape = getattr(data, "shape", None)
    if shape is None:
        cai = getattr(data, "__cuda_array_interface__", None)
        shape = cai["shape"] if cai is not None else None
    return int(shape[0]) if shape is not None and len(shape) > 0 else len(data)


def _n_shape(a):
    """Shape of a device array without touching it."""
    shape = getattr(a, "shape", None)
    return tuple(shape) if shape is not None else tuple(a.__cuda_array_interface__["shape"])


def _is_device_array(a):
    if type(a).__module__.split(".")[0] == "torch":
        return bool(getattr(a, "is_cuda", False))
    return getattr(a, "__cuda_array_interface__", None) is not None


def _check_sample_weight(sample_weight, n_rows, device_rows):
    """``train``'s ``sample_weight`` validated against ``n_rows`` rows, before any engine exists (``ValueError`` otherwise):
    one dimension, one value per row, a real dtype, every value finite and >= 0.  Returns a float32 host array -- or, for
    weights that live in HBM next to device rows, the device array itself (a 1-D torch CUDA tensor or
    ``__cuda_array_interface__`` object; its shape and dtype are checked here, its contents are the caller's business)."""
    if _is_device_array(sample_weight):
        if type(sample_weight).__module__.split(".")[0] == "torch":
            shape, real = tuple(sample_weight.shape), not (sample_weight.is_complex() or sample_weight.dtype == __import__("torch").bool)
        else:
            cai = sample_weight.__cuda_array_interface__
            shape, real = tuple(cai["shape"]), cai["typestr"] == "<f4" and cai.get("strides") is None
            if not real:
                raise ValueError('device sample_weight must be a C-contiguous float32 array')
        if len(shape) != 1:
            raise ValueError('sample_weight must be 1-dimensional, got shape %r' % (shape,))
        if shape[0] != n_rows:
            raise ValueError('sample_weight has %d values for %d rows of data' % (shape[0], n_rows))
        if not real:
            raise ValueError('sample_weight must have a real dtype, got %s' % (sample_weight.dtype,))
        if device_rows:
            return sample_weight
        if not hasattr(sample_weight, "cpu"):
            raise ValueError('sample_weight in device memory needs data in device memory')
        sample_weight = sample_weight.detach().cpu().numpy()       # host rows: the weights join them on the host
    w = np.asarray(sample_weight)
    if w.ndim != 1:
        raise ValueError('sample_weight must be 1-dimensional, got shape %r' % (w.shape,))
    if len(w) != n_rows:
        raise ValueError('sample_weight has %d values for %d rows of data' % (len(w), n_rows))
    if w.dtype == np.bool_ or not (np.issubdtype(w.dtype, np.integer) or np.issubdtype(w.dtype, np.floating)):
        raise ValueError('sample_weight must have a real dtype, got %s' % (w.dtype,))
    with np.errstate(over='ignore'):
        w32 = np.ascontiguousarray(w, dtype=np.float32)
    bad = np.flatnonzero(~(np.isfinite(w32) & (w32 >= 0)))          # (as float32: what the device will hold)
    if len(bad):
        raise ValueError('sample_weight must be finite and >= 0: sample_weight[%d] is %r' % (bad[0], w[bad[0]].item()))
    return w32


def _device_weights(w):
    """(pointer, device_index, owner, stream) of 1-D device weights as contiguous float32 (see _device_rows)."""
    if type(w).__module__.split(".")[0] == "torch":
        import torch
        t = w.detach()
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        torch.cuda.current_stream(t.device).synchronize()
        return t.data_ptr(), t.device.index, t, "done"
    cai = w.__cuda_array_interface__
    return int(cai["data"][0]), None, w, cai.get("stream")


def _host_rows(x, engine=None):
    """float32 host view of array-like input; device rows are copied back through ``engine()`` (analysis
    calls only; the engine is not created for host input)."""
    if hasattr(x, "is_cuda") and getattr(x, "is_cuda"):
        x = x.detach().cpu().numpy()
    elif getattr(x, "__cuda_array_interface__", None) is not None:
        ptr, n, d, _, _, stream = _device_rows(x)
        if engine is None:
            raise TypeError("device rows need an engine to be copied back to the host")
        eng = engine()
        eng.sync_producer(stream)
        return eng.copy_to_host(ptr, (n, d))
    return np.asarray(x, dtype=np.float32)


def units_adjacent(b1, b2, X, Y, topology):
    """Are the units with raveled ids b1 and b2 (arrays, id = i * Y + j) neighbours on an X x Y map?  topographic_error's
    adjacency rule, a pure function of the ids and the lattice.
      rectangular  |di| <= 1 and |dj| <= 1 (xpysom.py:709-746, rectangular branch)
      toroidal     the same on the wrapped offsets: |d| taken as min(|d|, L - |d|) per axis
      hexagonal    no farther apart than 1.5 in the hexagonal coordinates (xpysom.py:739-746).  The reference reads them
                   as _xx[i, j], _yy[i, j] from its UNtransposed (Y, X) meshgrids, i.e. x = j - s(i)/2, y = i with s
                   marking every second row from the last (xpysom.py:201-206) -- reproduced on square maps (pinned by
                   tests/golden/g13); on a non-square map that indexing runs out of bounds in the reference, and the
                   unit's own coordinates x = i - s(j)/2, y = j are used instead (deviations)."""
    b1, b2 = np.asarray(b1), np.asarray(b2)
    i1, j1, i2, j2 = b1 // Y, b1 % Y, b2 // Y, b2 % Y
    if topology == 'hexagonal':
        if X == Y:
            x1, y1 = j1 - 0.5 * ((Y - 1 - i1) % 2 == 0), i1
            x2, y2 = j2 - 0.5 * ((Y - 1 - i2) % 2 == 0), i2
        else:
            x1, y1 = i1 - 0.5 * ((Y - 1 - j1) % 2 == 0), j1
            x2, y2 = i2 - 0.5 * ((Y - 1 - j2) % 2 == 0), j2
        return ~(np.hypot(x1 - x2, (y1 - y2).astype(float)) > 1.5)
    di, dj = np.abs(i1 - i2), np.abs(j1 - j2)
    if topology == 'toroidal':
        di, dj = np.minimum(di, X - di), np.minimum(dj, Y - dj)
    return ~((di > 1) | (dj > 1))


EpochRecord = namedtuple('EpochRecord', ['iteration', 'sigma', 'learning_rate', 'quantization_error', 'rows', 'weight',
                                         'bmu_changed', 'codebook_shift', 'codebook_shift_max'])
EpochRecord.__doc__ = """What a monitored epoch of ``XPySom.train`` / ``train_streaming`` appends to ``XPySom.history``: plain Python
numbers.  The epoch ran with codebook W_t and produced W_t+1.
  iteration, sigma, learning_rate   what the epoch was run with
  quantization_error   sum_n w_n d_n / sum_n w_n over the rows of weight > 0 (all rows, w_n = 1, without sample weights): d_n the
                       float32 Euclidean distance of row n to W_t[b_n], b_n the BMU the epoch's OWN search found under the
                       configured distance and precision; with missing='nan' over the observed features.  NaN when the weights
                       sum to 0 (no rows).  Not ``quantization_error(data)`` bit for bit: that call searches under the sqrt'd
                       Euclidean distance (ties can fall differently), and under the cosine, Manhattan and norm_p distances the
                       epoch's unit is a different unit altogether
  rows, weight         rows measured (weight > 0) and the sum of their weights, over all ranks
  bmu_changed          rows whose BMU differs from the previous monitored epoch's over the same resident rows; None for the first
                       monitored epoch of a ``train`` call and for every streamed epoch
  codebook_shift       sqrt(sum (W_t+1 - W_t)^2) over all units and features; codebook_shift_max the largest |W_t+1 - W_t|"""


def _check_monitor(monitor, callback):
    """``train``'s ``monitor`` / ``callback`` validated before any engine exists; returns whether the schedule is monitored."""
    if not isinstance(monitor, (bool, np.bool_)):
        raise TypeError('monitor must be a bool, got %r' % (monitor,))
    if callback is not None and not callable(callback):
        raise TypeError('callback must be callable or None, got %r' % (callback,))
    return bool(monitor) or callback is not None


def _epoch_record(iteration, sig, eta, m):
    """The EpochRecord of one monitored epoch from the metrics ``distributed.epoch`` filled in."""
    qe = m['sum_wd'] / m['sum_w'] if m['sum_w'] != 0 else float('nan')
    return EpochRecord(int(iteration), float(sig), float(eta), float(qe), int(m['rows']), float(m['sum_w']),
                       int(m['changed']) if m['changed'] >= 0 else None, float(np.sqrt(m['shift_sumsq'])),
                       float(m['shift_max']))


class UnitStatistics:
    """What ``XPySom.unit_statistics`` returns: per unit of an ``(x, y)`` map, over the samples the unit wins,
    ``hits`` (int64), ``sum`` and ``sumsq`` of their distances to it (float64) and ``max`` (float32; 0 for a unit without
    samples).  ``hits``, ``sum`` and ``sumsq`` are the raw additive quantities: shards or ranks add them (``max``: the
    elementwise maximum) and derive ``mean`` and ``std`` afterwards."""

    def __init__(self, hits, sum, sumsq, max):
        self.hits, self.sum, self.sumsq, self.max = hits, sum, sumsq, max

    @property
    def mean(self):
        """Mean distance per unit, the quantization-error map; NaN where the unit has no samples."""
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(self.hits == 0, np.nan, self.sum / self.hits)

    @property
    def std(self):
        """Population standard deviation of the distances per unit, sqrt(max(sumsq / hits - mean^2, 0)); NaN where the unit
        has no samples."""
        with np.errstate(divide='ignore', invalid='ignore'):
            var = self.sumsq / self.hits - self.mean ** 2
            return np.where(self.hits == 0, np.nan, np.sqrt(np.maximum(var, 0.0)))

    def __repr__(self):
        return "UnitStatistics(%d x %d units, %d samples)" % (self.hits.shape + (int(self.hits.sum()),))


class UnitMeans:
    """What ``XPySom.unit_means`` returns: per unit of an ``(x, y)`` map and column of the values, over the samples the unit
    wins whose value in the column is not NaN, ``count`` (int64), ``sum`` and ``sumsq`` (float64), ``(x, y, n_cols)`` arrays.
    They are the raw additive quantities: shards or ranks add them and derive ``mean`` and ``std`` afterwards."""

    def __init__(self, count, sum, sumsq):
        self.count, self.sum, self.sumsq = count, sum, sumsq

    @property
    def mean(self):
        """Mean of every column per unit, the component plane of a variable the map was not trained on; NaN where the unit
        observed no value of the column."""
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(self.count == 0, np.nan, self.sum / self.count)

    @property
    def std(self):
        """Population standard deviation per unit and column, sqrt(max(sumsq / count - mean^2, 0)); NaN where the unit
        observed no value of the column."""
        with np.errstate(divide='ignore', invalid='ignore'):
            var = self.sumsq / self.count - self.mean ** 2
            return np.where(self.count == 0, np.nan, np.sqrt(np.maximum(var, 0.0)))

    def __repr__(self):
        return "UnitMeans(%d x %d units, %d columns)" % self.count.shape


def _device_column(a, dtype_name, typestr):
    """(pointer, shape, device_index, owner, stream) of labels or values that live in HBM next to device rows, as a contiguous
    array of the dtype the engine reads (see _device_rows)."""
    if type(a).__module__.split(".")[0] == "torch":
        import torch
        t, want = a.detach(), getattr(torch, dtype_name)
        if t.dtype != want or not t.is_contiguous():
            t = t.to(want).contiguous()
        torch.cuda.current_stream(t.device).synchronize()
        return t.data_ptr(), tuple(t.shape), t.device.index, t, "done"
    cai = a.__cuda_array_interface__
    if cai["typestr"] != typestr or cai.get("strides") is not None:
        raise ValueError('device %s must be a C-contiguous %s array' % ('labels' if dtype_name == 'int32' else 'values', dtype_name))
    return int(cai["data"][0]), tuple(cai["shape"]), None, a, cai.get("stream")


def _to_device(host, device_index):
    """A host array copied next to device rows (torch is the plumbing for device memory here)."""
    import torch
    return torch.from_numpy(host).to(torch.device("cuda", device_index))


def _nan_init_message(what):
    return "%s: the data holds NaN (missing values); initialise from complete rows" % what


def _pca_codebook(cov, x, y):
    """The reference's PCA codebook (xpysom.py:779-785) of a covariance matrix, (x, y, D): its own ``np.linalg.eig``, its own
    formula -- ROWS of the eigenvector matrix, no mean, no scale --, one broadcast over the grid in place of the loop over the
    units: the same elementwise arithmetic, hence the same bits."""
    pc_length, pc = np.linalg.eig(cov)
    order = np.argsort(-pc_length)
    c1 = np.linspace(-1, 1, x)[:, None, None]
    c2 = np.linspace(-1, 1, y)[None, :, None]
    return c1 * pc[order[0]][None, None, :] + c2 * pc[order[1]][None, None, :]


def _linear_codebook(wsum, mean, cov, x, y):
    """The linear initialisation (the SOM Toolbox's ``lininit``) of an x * y map from weighted moments, (x, y, D) float64:
    ``W[i, j] = mean + c_i sqrt(l1) v1 + c_j sqrt(l2) v2``, (l, v) the two leading eigenpairs of ``np.linalg.eigh(cov)`` (l clipped at
    0), the FIRST axis along the longer side of the map (a tie: along x), coordinates ``linspace(-1, 1, side)`` (a side of 1: 0), and
    every vector's sign fixed so that its first largest-magnitude component is positive.  ``wsum``: the weights' sum the moments
    were divided by, which must be positive."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    if not wsum > 0:
        raise ValueError('linear_weights_init: the sample weights sum to 0')
    if not (np.isfinite(mean).all() and np.isfinite(cov).all()):
        raise ValueError(_nan_init_message('linear_weights_init'))
    lam, vec = np.linalg.eigh(cov)                       # ascending
    axes = []
    for k in (-1, -2):
        v = vec[:, k]
        if v[np.argmax(np.abs(v))] < 0:                  # (argmax: the first of equal magnitudes)
            v = -v
        axes.append(np.sqrt(max(lam[k], 0.0)) * v)
    cx = np.linspace(-1, 1, x) if x > 1 else np.zeros(1)
    cy = np.linspace(-1, 1, y) if y > 1 else np.zeros(1)
    ax, ay = (axes[0], axes[1]) if x >= y else (axes[1], axes[0])
    return mean[None, None, :] + cx[:, None, None] * ax[None, None, :] + cy[None, :, None] * ay[None, None, :]


def _ustar(u, p):
    """Ultsch's U*-matrix from a U-matrix ``u`` and a P-matrix ``p`` of the same shape, float64:
    ``U* = U * ((P - mean P) / (mean P - max P) + 1)`` -- ``U`` where the density is the mean, 0 where it is the maximum.  A flat
    density (``max P == mean P``) returns ``U`` unchanged."""
    u = np.asarray(u, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    if u.shape != p.shape:
        raise ValueError("the U-matrix is %r, the P-matrix %r" % (u.shape, p.shape))
    mean, top = p.mean(), p.max()
    if top == mean:
        return u.copy()
    return u * ((p - mean) / (mean - top) + 1.0)


def _sdh(rank_counts):
    """Pampalk's smoothed data histogram from the rank counts ``(s, ...)``: rank j weighs ``(s - j) / (s (s + 1) / 2)``."""
    c = np.asarray(rank_counts, dtype=np.float64)
    s = c.shape[0]
    out = np.zeros(c.shape[1:], dtype=np.float64)
    for j in range(s):                                   # (rank by rank, in order: one result on every NumPy)
        out += c[j] * ((s - j) / (s * (s + 1) / 2.0))
    return out


class XPySom:
    def __init__(self, x, y, input_len,
                 sigma=0, sigmaN=1,
                 learning_rate=0.5, learning_rateN=0.01, decay_function='exponential',
                 neighborhood_function='gaussian', std_coeff=0.5,
                 topology='rectangular',
                 activation_distance='euclidean',
                 activation_distance_kwargs={},
                 random_seed=None, n_parallel=0, compact_support=False,
                 xp=None,
                 use_dask=False, dask_chunks='auto',
                 *, precision='exact', device=None, sharded_input=False, shard='contiguous', missing=None):
        """Same positional/keyword surface as the reference constructor (xpysom.py:73-82).

        ``xp``, ``use_dask`` and ``dask_chunks`` are accepted for source compatibility and
        ignored: there is one backend (HIP) and multi-GPU runs use torch.distributed, not Dask.
        Extra keyword-only arguments:
          precision      'exact' (the DEFAULT: the BMUs of 'f32' bit for bit -- hence its accumulators and its trained
                         codebook --, found by an IEEE-half MFMA screen and a float32 re-score of the units its error
                         bound cannot rule out; where no screen applies -- small maps, the VALU distances -- the float32
                         kernels themselves serve it), 'f32' (the exact-float32 MFMA kernels over every unit: the parity
                         mode the default is checked against), 'bf16' (bf16 MFMA distance GEMM: BMUs within the operand
                         rounding of float32's), or the same path on IEEE half operands, 'f16' (three more mantissa bits
                         at the same MFMA rate; rows and units must fit float16: norms <= 65504)
          device         HIP device ordinal (default: LOCAL_RANK or 0)
          sharded_input  under an initialised process group: ``train(data)`` receives only this
                         rank's rows (default: every rank passes the full array and takes its slice)
          shard          which slice that is: 'contiguous' (rows [lo, hi): the reference's Dask blocks, xpysom.py:490,546)
                         or 'strided' (rows rank, rank + world, ...: every rank a sample of the whole file, so that an
                         order in the input cannot become rank skew under block skipping); the same map either way, to
                         float32 summation order
          missing        None (the default: a NaN is a value like any other, and poisons what it touches) or 'nan': a NaN
                         in training, streamed or query rows means "not observed".  The BMU of a row is the first minimum
                         of the squared distance over its observed features (a row with none takes unit 0 and teaches
                         nothing); the batch update keeps a numerator and a denominator per unit AND feature,
                         W[k, d] = sum_n g m_nd x_nd / sum_n g m_nd, and leaves W[k, d] untouched where no observed value
                         reached it; quantization_error is the mean over all rows of the distance over the observed
                         features.  The codebook never receives a NaN from the data.  'euclidean' only, precision 'exact'
                         or 'f32' (both run the float32 masked kernel); every neighbourhood and topology; train (with
                         sample_weight, device rows), train_streaming, winner, predict, quantization, quantization_error,
                         activation_response, win_map, labels_map, impute (every NaN of a row replaced by its best matching
                         unit's value for that feature).  topographic_error, activate, distance_from_weights,
                         density_map, ustar_map, nearest_units, rank_hits and smoothed_hits raise
                         NotImplementedError; the initialisers refuse data with a NaN
        """
        if sigma >= x or sigma >= y:
            warn('Warning: sigma is too high for the dimension of the map.')

        self._random_generator = np.random.RandomState(random_seed)
        self.use_dask = False
        self.dask_chunks = dask_chunks

        self._learning_rate = learning_rate
        self._learning_rateN = learning_rateN
        self._sigma = min(x, y) / 2 if sigma == 0 else sigma
        self._std_coeff = std_coeff
        self._sigmaN = sigmaN
        self._input_len = input_len

        # seeded default codebook, float64 on the host exactly as xpysom.py:189-190
        self._weights = self._random_generator.rand(x, y, input_len) * 2 - 1
        self._weights /= np.linalg.norm(self._weights, axis=-1, keepdims=True)

        self._neigx = np.arange(x)
        self._neigy = np.arange(y)

        if topology not in TOPOLOGIES:
            msg = '%s not supported only hexagonal and rectangular available'
            raise ValueError(msg % topology)
        self.topology = topology

        if decay_function not in DECAY_FUNCTIONS:
            msg = '%s not supported. Functions available: %s'
            raise ValueError(msg % (decay_function, ', '.join(DECAY_FUNCTIONS.keys())))
        self._decay_function = DECAY_FUNCTIONS[decay_function]
        self._decay_function_name = decay_function

        self.compact_support = compact_support
        available = [n for n in NEIGHBORHOODS if not (topology == 'hexagonal' and n == 'triangle')]
        if neighborhood_function not in available:
            msg = '%s not supported. Functions available: %s'
            raise ValueError(msg % (neighborhood_function, ', '.join(available)))
        self.neighborhood_func_name = neighborhood_function

        if activation_distance not in DISTANCES:
            msg = '%s not supported. Distances available: %s'
            raise ValueError(msg % (activation_distance, ', '.join(DISTANCES.keys())))
        self._activation_distance_name = activation_distance
        self._activation_distance_kwargs = activation_distance_kwargs

        if not DISTANCES[activation_distance]:
            raise NotImplementedError("activation_distance '%s' is not in the HIP engine yet "
                                      "(SURVEY 8(f) rank 3)" % activation_distance)
        if precision in ('bf16x3', 'f16x3'):
            raise ValueError("precision '%s' is retired: 'exact' returns float32's own BMUs, faster" % precision)
        if precision not in ('f32', 'exact', 'bf16', 'f16'):
            raise ValueError("precision must be 'exact', 'f32', 'bf16' or 'f16'")
        # what som_create would refuse is refused here, at construction, as the reference raises at
        # construction (the engine itself is created lazily, on the first train() / winner())
        if neighborhood_function == 'mexican_hat' and compact_support and topology == 'rectangular' and x != y:
            # the reference masks px twice and py never (neighborhoods.py:69-71); its second mask is an (n, y) array
            # against px's (n, x), so NumPy refuses to broadcast it at the first _update.  Reproduced on square maps.
            raise ValueError('mexican_hat with compact_support needs a square map on the rectangular topology: '
                             'operands could not be broadcast together with shapes (n,%d) (n,%d)' % (x, y))
        if neighborhood_function == 'mexican_hat' and compact_support and topology == 'toroidal':
            # the rectangular form exists to reproduce the reference's double mask; the torus has no reference to reproduce
            raise ValueError('mexican_hat with compact_support is not defined on the toroidal topology')
        if precision not in ('f32', 'exact') and activation_distance not in ('euclidean', 'cosine'):
            raise ValueError("precision '%s' implements the GEMM-form distances 'euclidean' and 'cosine'; "
                             "'%s' needs precision='f32'" % (precision, activation_distance))
        if activation_distance.startswith('norm_p'):
            p = activation_distance_kwargs.get('p', 2)
            if isinstance(p, (int, np.integer)) or (isinstance(p, (float, np.floating)) and float(p).is_integer()):
                if not 1 <= int(p) <= 16:
                    raise NotImplementedError("norm_p: an integer exponent p must be in 1..16, got %r" % (p,))
            elif isinstance(p, (float, np.floating)):
                # a real exponent (distances.py:61-75 takes any p): the generic |x - w|^p form
                if not (np.isfinite(p) and 0.0 < float(p) <= 64.0):
                    raise NotImplementedError("norm_p: a real exponent p must be in (0, 64], got %r" % (p,))
            else:
                raise NotImplementedError("norm_p: the exponent p must be a number, got %r" % (p,))

        # n_parallel bounded the (n,K) temporaries of the reference (xpysom.py:242-251); nothing of
        # that size exists here, it only sizes host->device staging of winner()/quantization_error().
        if n_parallel == 0:
            n_parallel = DEFAULT_BATCH_ROWS
        self._n_parallel = n_parallel

        if missing not in (None, 'nan'):
            raise ValueError("missing must be None or 'nan', got %r" % (missing,))
        if missing == 'nan':
            if activation_distance != 'euclidean':
                raise ValueError("missing='nan' is defined for activation_distance='euclidean' only, got '%s'" % activation_distance)
            if precision not in ('f32', 'exact'):
                raise ValueError("missing='nan' runs the float32 masked kernel: precision 'exact' or 'f32', not '%s'" % precision)
        self._missing = missing
        self._precision = precision
        self._device = device
        self._sharded_input = sharded_input
        if shard not in _dist.SHARDS:
            raise ValueError("shard must be one of %s" % ", ".join(_dist.SHARDS))
        self._shard = shard
        self._engine_obj = None
        self.history = []                    # EpochRecords of the monitored epochs so far (train(..., monitor=True)); never cleared here

    # ------------------------------------------------------------------ engine plumbing
    def _engine(self):
        if self._engine_obj is None:
            x, y, _ = self._weights.shape
            kw = dict(distance=self._activation_distance_name, neighborhood=self.neighborhood_func_name,
                      std_coeff=self._std_coeff, compact_support=self.compact_support,
                      precision=self._precision, topology=self.topology)
            if getattr(self, '_missing', None) is not None:
                kw['missing'] = self._missing
            if self._activation_distance_name.startswith('norm_p'):
                p = self._activation_distance_kwargs.get('p', 2)
                if isinstance(p, (float, np.floating)) and not float(p).is_integer():
                    kw['norm_p'], kw['norm_p_real'] = 2, float(p)
                else:
                    kw['norm_p'] = int(p)
            from . import engine
            dev = self._device
            if dev is None:
                import os
                dev = int(os.environ.get('LOCAL_RANK', '0'))
            self._engine_obj = engine.HipEngine(x, y, self._input_len, device=dev, **kw)
        return self._engine_obj

    def _upload_weights(self):
        eng = self._engine()
        eng.set_weights(np.asarray(self._weights, dtype=np.float32))
        return eng

    def get_weights(self):
        """Returns the weights of the neural network."""
        return self._weights

    def get_euclidean_coordinates(self):
        """Meshgrids (xx, yy) of the units' positions on the euclidean plane of the chosen topology:
        unit (i, j) sits at (xx[i, j], yy[i, j]) (xpysom.py:291-305)."""
        xx, yy = np.meshgrid(self._neigx, self._neigy)
        xx, yy = xx.astype(float), yy.astype(float)
        if self.topology == 'hexagonal':
            xx[::-2] -= 0.5
        return xx.T, yy.T

    def convert_map_to_euclidean(self, xy):
        """Map coordinates -> euclidean coordinates of the chosen topology (xpysom.py:308-320)."""
        xx, yy = self.get_euclidean_coordinates()
        return xx[xy], yy[xy]

    def activate(self, x):
        """Activation map of x: its distance to every unit under the configured distance, shape (n, K)
        (xpysom.py:323-354).  An analysis call: training never materialises this matrix."""
        self._refuse_missing('activate')
        x = _host_rows(x, self._engine)
        if x.ndim == 0:
            x = x.reshape(1, 1)
        elif x.ndim == 1:
            x = x[None, :]
        if self._activation_distance_name not in ('euclidean', 'euclidean_no_opt', 'cosine'):
            raise NotImplementedError("activate() returns the (n, K) matrix of the GEMM-form distances only; '%s' is "
                                      "a fused distance+argmin kernel here (use winner())" % self._activation_distance_name)
        return self._upload_weights().distance_matrix(x)

    def distance_from_weights(self, data, weights_gpu=None):
        """d[i, j] = euclidean distance between data[i] and the j-th unit (xpysom.py:647-671)."""
        self._refuse_missing('distance_from_weights')
        data = _host_rows(data, self._engine)
        return self._upload_weights().distance_matrix(data, quantization=True)

    def distance_map(self):
        """U-matrix: each unit's summed distance to its map neighbours, scaled to a maximum of 1
        (xpysom.py:788-817: 8 neighbours on the rectangular grid; 6 on the hexagonal one, whose offsets
        depend on the parity of the unit's column index j; on the toroidal one the 8 offsets applied cyclically, so
        every unit has all 8 -- on a side of 1 or 2 an offset may lead to the unit itself or to the same neighbour
        twice, and counts as often).  One shifted difference per neighbour offset over the whole codebook --
        host-side, the codebook is tiny next to the data."""
        w = np.asarray(self._weights, dtype=np.float64)
        X, Y = w.shape[:2]
        if self.topology == 'toroidal':
            um = np.zeros((X, Y))
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if (di, dj) != (0, 0):      # np.roll(w, -d)[x] = w[(x + d) % L]
                        um += np.linalg.norm(w - np.roll(w, (-di, -dj), axis=(0, 1)), axis=-1)
            return um / um.max()
        if self.topology == 'hexagonal':
            offsets = {1: ((0, 1), (1, 0), (0, -1), (-1, -1), (-1, 0), (-1, 1)),      # even j
                       0: ((1, 1), (1, 0), (1, -1), (0, -1), (-1, 0), (0, 1))}        # odd j
        else:
            ring = tuple((di, dj) for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0))
            offsets = {0: ring, 1: ring}
        um = np.zeros((X, Y))
        even = (np.arange(Y) % 2 == 0)[None, :]
        for parity, offs in offsets.items():
            for di, dj in offs:
                # units (x, y) with an in-range neighbour (x + di, y + dj)
                xs = slice(max(0, -di), X - max(0, di))
                ys = slice(max(0, -dj), Y - max(0, dj))
                xn = slice(max(0, di), X - max(0, -di))
                yn = slice(max(0, dj), Y - max(0, -dj))
                d = np.linalg.norm(w[xs, ys] - w[xn, yn], axis=-1)
                um[xs, ys] += d * (even[:, ys] == bool(parity))
        return um / um.max()

    def _refuse_missing(self, what):
        if getattr(self, '_missing', None) is not None:
            raise NotImplementedError("%s() is not defined with missing='%s': a distance over a row's observed features has no "
                                      "common scale across rows" % (what, self._missing))

    def _refuse_nan_init(self, what, data):
        if getattr(self, '_missing', None) is not None and np.isnan(np.asarray(data, dtype=np.float64)).any():
            raise ValueError(_nan_init_message(what))

    def _check_input_len(self, data):
        """Checks that the data in input is of the correct shape (xpysom.py:360-366)."""
        data_len = len(data[0])
        if self._input_len != data_len:
            msg = 'Received %d features, expected %d.' % (data_len, self._input_len)
            raise ValueError(msg)

    # ------------------------------------------------------------------ training
    def train(self, data, num_epochs, iter_beg=0, iter_end=None, verbose=False, *, sample_weight=None, monitor=False,
              callback=None):
        """Trains the SOM (batch algorithm); same contract as xpysom.py:458-594.

        ``sample_weight`` (keyword-only; not in the reference) gives the rows unequal importance: one finite value >= 0
        per row of ``data``; a row of weight w adds w times its features to its BMU's sum and w to its count -- an
        integer weight m is the row repeated m times, a weight of 0 leaves the row out (its features are not read).  The
        BMU search does not see the weights.  A host array-like, or next to device rows a device array on the same
        device.  Under a process group the weights are cut like the rows.  An argument of this call, not state: a later
        ``train`` without it is unweighted.

        ``monitor=True`` (keyword-only; not in the reference) appends an ``EpochRecord`` per epoch to ``self.history`` (a plain
        list the library never clears): the epoch's quantization error under its own BMUs, how many rows changed BMU, how far
        the codebook moved -- measured on the device from what the epoch itself left there, for two small launches and one
        host synchronisation per epoch; the trained codebook is the unmonitored one bit for bit.  ``callback(record)`` (implies
        ``monitor``) runs after each epoch's merge; a truthy return ends the schedule there, with the codebook and the records
        of the epochs that completed.  Under a process group every rank holds the same record, so a callback that is a pure
        function of the record stops every rank at the same epoch.

        ``iter_beg``/``iter_end`` resume the schedule mid-run (decays are pure functions of
        (iteration, num_epochs)).  Under an initialised torch.distributed group the rows are
        sharded contiguously over the ranks and the per-epoch numerator/denominator are
        all-reduced before the merge.  Returns ``self``; ``_weights`` is float32 afterwards."""
        if iter_end is None:
            iter_end = num_epochs
        monitored = _check_monitor(monitor, callback)    # (refused before an engine exists)

        rank, world = _dist.dist_info()
        on_device = _device_rows(data) is not None
        if not on_device:
            data = np.asarray(data, dtype=np.float32)
            if data.ndim != 2:
                raise ValueError('data must be 2-dimensional (n_samples, input_len)')
        weights = None
        if sample_weight is not None:                    # refused here, before an engine (or a GPU) is needed
            weights = _check_sample_weight(sample_weight, _n_rows(data), on_device)
            if world > 1 and not self._sharded_input:    # cut like the rows: weight i stays with row i
                weights = _dist.shard_rows(weights, rank, world, getattr(self, '_shard', 'contiguous'))
        if on_device:                                    # rows already in HBM: no host round trip
            if world > 1 and not self._sharded_input:
                data = _dist.shard_rows(data, rank, world, getattr(self, '_shard', 'contiguous'))
            ptr, n, d, dev_index, owner, stream = _device_rows(data)
            eng = self._upload_weights()
            if dev_index is not None and dev_index != eng.device:
                raise ValueError('device data lives on cuda:%d, the engine on cuda:%d' % (dev_index, eng.device))
            if d != self._input_len:
                raise ValueError('Received %d features, expected %d.' % (d, self._input_len))
            if stream != "done":                         # rows of a foreign producer: wait for its stream (or the device)
                eng.sync_producer(stream)
            eng.set_data_device(ptr, n, keepalive=owner)
        else:
            if world > 1 and not self._sharded_input:
                data = _dist.shard_rows(data, rank, world, getattr(self, '_shard', 'contiguous'))
            eng = self._upload_weights()
            eng.set_data(data)
        # (set_data* has dropped any earlier call's weights: without sample_weight this call is the unweighted one)
        if weights is not None and _is_device_array(weights):
            wptr, wdev, wowner, wstream = _device_weights(weights)
            if wdev is not None and wdev != eng.device:
                raise ValueError('sample_weight lives on cuda:%d, the engine on cuda:%d' % (wdev, eng.device))
            if wstream != "done":
                eng.sync_producer(wstream)
            eng.set_sample_weights_device(wptr, eng.n_rows, keepalive=wowner)
        elif weights is not None:
            eng.set_sample_weights(weights)
        if monitored:
            eng.monitor(True)
        elif getattr(eng, 'monitoring', False):          # an earlier monitored call's: an unmonitored schedule launches nothing for it
            eng.monitor(False)

        try:
            for iteration in range(iter_beg, iter_end):
                eta = self._decay_function(self._learning_rate, self._learning_rateN, iteration, num_epochs)
                # sigma and learning rate decrease with the same rule
                sig = self._decay_function(self._sigma, self._sigmaN, iteration, num_epochs)
                # NumPy >= 2: a numpy scalar sigma makes the reference's neighbourhood float64
                neigh_f64 = isinstance(sig, np.generic)
                self._check_sigma(sig)
                if monitored:
                    m = {}
                    _dist.epoch(eng, sig, eta, neigh_f64, metrics=m)
                    record = _epoch_record(iteration, sig, eta, m)
                    self.history.append(record)
                else:
                    _dist.epoch(eng, sig, eta, neigh_f64)
                if verbose:
                    print('\r [ %d / %d ] %3.0f%%' % (iteration + 1, num_epochs, 100 * (iteration + 1) / num_epochs),
                          end='')
                if callback is not None and callback(record):
                    break
        finally:
            # also on the way out of an exception (mexican_hat's ZeroDivisionError at sigma 0): the object holds
            # the codebook of the epochs that completed, as the reference's does
            self._weights = eng.get_weights().reshape(self._weights.shape)

        if verbose:
            print('\n quantization error:', self.quantization_error(data))
        return self

    def _check_sigma(self, sig):
        """mexican_hat evaluates ``1 - 2/d*p`` with ``d = 2*std_coeff**2*sigma**2`` (neighborhoods.py:72, :94): a
        Python-float sigma of exactly 0 -- a linear schedule ending at sigmaN=0 -- raises there, in the reference, and
        so here (a numpy.float64 sigma divides to inf with a warning; the gaussian's 0/0 gives NaN in both)."""
        if self.neighborhood_func_name == 'mexican_hat' and not isinstance(sig, np.generic) \
                and 2 * self._std_coeff ** 2 * sig ** 2 == 0:    # d, associated as neighborhoods.py:59 writes it
            raise ZeroDivisionError('float division by zero')

    def train_streaming(self, chunks, num_epochs, iter_beg=0, iter_end=None, *, monitor=False, callback=None):
        """``train`` for data that does not stay resident in HBM (or in host memory as one array).

        ``chunks`` is a callable returning a fresh iterable of ``(n_i, input_len)`` row blocks for each
        epoch (e.g. slices of a ``numpy.memmap``) -- the role Dask blocks play in the reference
        (xpysom.py:545-556).  A block may also be a ``(rows, weights)`` pair with one sample weight per row
        (``train``'s ``sample_weight``); an epoch's blocks are all of one form or all of the other (``ValueError``).  Every block goes host -> HBM, through the BMU kernel and into the same
        segment sums; the epoch ends with the usual transform, all-reduce and merge.  Under a process
        group each rank streams its own blocks.

        ``monitor`` and ``callback`` as in ``train``: every block is measured behind its own BMU search, an epoch's sums are
        added in block order; ``bmu_changed`` is always None (no rows stay to compare)."""
        if iter_end is None:
            iter_end = num_epochs
        monitored = _check_monitor(monitor, callback)
        eng = self._upload_weights()
        if monitored:
            eng.monitor(True)
        elif getattr(eng, 'monitoring', False):          # an earlier monitored call's: an unmonitored schedule launches nothing for it
            eng.monitor(False)
        try:
            for iteration in range(iter_beg, iter_end):
                eta = self._decay_function(self._learning_rate, self._learning_rateN, iteration, num_epochs)
                sig = self._decay_function(self._sigma, self._sigmaN, iteration, num_epochs)
                self._check_sigma(sig)
                if monitored:
                    m = {}
                    _dist.epoch(eng, sig, eta, isinstance(sig, np.generic), chunks=chunks(), metrics=m)
                    record = _epoch_record(iteration, sig, eta, m)
                    self.history.append(record)
                    if callback is not None and callback(record):
                        break
                else:
                    _dist.epoch(eng, sig, eta, isinstance(sig, np.generic), chunks=chunks())
        finally:
            self._weights = eng.get_weights().reshape(self._weights.shape)
        return self

    def train_batch(self, data, num_iteration, verbose=False):
        """Compatibility with MiniSom, alias for train"""
        return self.train(data, num_iteration, verbose=verbose)

    def train_random(self, data, num_iteration, verbose=False):
        """Compatibility with MiniSom, alias for train"""
        print("WARNING: due to batch SOM algorithm, random order is not supported. Falling back to train_batch.")
        return self.train(data, num_iteration, verbose=verbose)

    # ------------------------------------------------------------------ inference
    def _device_query(self, x):
        """(engine, pointer, n_rows) for 2-D float32 rows that already live in HBM, else None: such rows are searched where
        they are (som_bmu_device), whole -- no host round trip, no n_parallel chunks (xpysom.py:379-396 on a CuPy array)."""
        shape = getattr(x, 'shape', None)
        if shape is None or len(shape) != 2:
            return None
        dev = _device_rows(x)
        if dev is None:
            return None
        ptr, n, d, dev_index, owner, stream = dev
        if d != self._input_len:
            raise ValueError('Received %d features, expected %d.' % (d, self._input_len))
        eng = self._upload_weights()
        if dev_index is not None and dev_index != eng.device:
            raise ValueError('device data lives on cuda:%d, the engine on cuda:%d' % (dev_index, eng.device))
        if stream != "done":
            eng.sync_producer(stream)
        return eng, ptr, n, owner

    def _ids_of(self, x, quantization=False):
        """Raveled BMU ids of host or device rows."""
        q = self._device_query(x)
        if q is not None:
            eng, ptr, n, _owner = q
            return eng.bmu_device(ptr, n, quantization=quantization)
        return self._winner_ids(_host_rows(x, self._engine), quantization=quantization)

    def _winner_ids(self, x2d, quantization=False):
        eng = self._upload_weights()
        out = [eng.bmu(x2d[s:s + self._n_parallel], quantization=quantization)
               for s in range(0, len(x2d), self._n_parallel)]
        return np.concatenate(out) if out else np.zeros(0, dtype=np.int32)

    def winner(self, x):
        """Coordinates of the winning neuron(s): ``(i, j)`` for one sample, a list of
        ``(i, j)`` tuples (numpy.int64) for a matrix -- xpysom.py:370-408."""
        # the reference does not coerce x (xpysom.py:379-396): float64 rows against trained (float32) weights are scored in
        # float64 by NumPy.  Served for the 'euclidean' distance in the float32-exact modes; elsewhere x is taken as float32
        x64 = None
        if (isinstance(x, np.ndarray) and x.dtype == np.float64 and np.asarray(self._weights).dtype == np.float32
                and self._activation_distance_name == 'euclidean' and self._precision in ('f32', 'exact')
                and getattr(self, '_missing', None) is None):
            x64 = x
        if self._device_query(x) is not None:               # rows in HBM: searched there
            ids = self._ids_of(x).astype(np.int64)
            wi, wj = np.divmod(ids, self._weights.shape[1])
            return list(map(tuple, np.vstack([wi, wj]).T))
        x = _host_rows(x, self._engine)
        one = x.ndim == 1
        if one:
            x = x[None, :]
        if x64 is not None:
            x64 = x64[None, :] if one else x64
            eng = self._upload_weights()
            ids = np.concatenate([eng.bmu_f64(x64[s:s + self._n_parallel])
                                  for s in range(0, len(x64), self._n_parallel)]).astype(np.int64) if len(x64) else np.zeros(0, np.int64)
        else:
            ids = self._winner_ids(x).astype(np.int64)
        wi, wj = np.divmod(ids, self._weights.shape[1])
        if one:
            return (wi[0].item(), wj[0].item())
        return list(map(tuple, np.vstack([wi, wj]).T))

    def quantization(self, data):
        """Assigns a code book (weights vector of the winning neuron) to each sample in data."""
        if self._device_query(data) is None:
            data = _host_rows(data, self._engine)
            self._check_input_len(data)
        ids = self._ids_of(data, quantization=True)
        w = np.asarray(self._weights)
        return w.reshape(-1, w.shape[2])[ids]

    def quantization_error(self, data):
        """Average distance between each input sample and its best matching unit
        (always Euclidean, xpysom.py:673-707).  Returns a Python float."""
        q = self._device_query(data)
        if q is not None:
            eng, ptr, n, _owner = q
            return eng.quantization_error_device(ptr, n) if n else float('nan')
        data = _host_rows(data, self._engine)
        self._check_input_len(data)
        eng = self._upload_weights()
        total, n = 0.0, 0
        for s in range(0, len(data), self._n_parallel):
            chunk = data[s:s + self._n_parallel]
            total += eng.quantization_error(chunk) * len(chunk)
            n += len(chunk)
        return total / n if n else float('nan')

    def _diag_query(self, data):
        """(engine, device query or None, host rows or None) for the map diagnostics: device rows stay where they are, host
        rows are coerced (a 1-D row is one sample) and their feature count is checked; the codebook is uploaded once."""
        q = self._device_query(data)
        if q is not None:
            return q[0], q, None
        data = _host_rows(data, self._engine)
        if data.ndim == 1:
            data = data[None, :]
        if len(data):
            self._check_input_len(data)
        return self._upload_weights(), None, data

    def quantization_distances(self, data):
        """``(ids, dist)``: every sample's best matching unit under the Euclidean distance (int64, raveled as in
        ``predict``) and its distance to it (float32) -- the per-sample terms ``quantization_error`` averages, and the usual
        novelty score of a sample.  Rows in HBM are searched where they are, whole; host rows in ``n_parallel`` chunks.
        With ``missing='nan'`` the distance runs over a row's observed features (a row with none: unit 0, distance 0)."""
        eng, q, data = self._diag_query(data)
        if q is not None:
            ids, dist = eng.bmu_distances_device(q[1], q[2]) if q[2] else (np.zeros(0, np.int32), np.zeros(0, np.float32))
            return ids.astype(np.int64), dist
        parts = [eng.bmu_distances(data[s:s + self._n_parallel]) for s in range(0, len(data), self._n_parallel)]
        if not parts:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
        return np.concatenate([p[0] for p in parts]).astype(np.int64), np.concatenate([p[1] for p in parts])

    def _impute_out(self, data, owner, ptr, n, out, eng):
        """(pointer, object to return) of ``impute``'s result for device rows: checked here, before the engine is called."""
        d = self._input_len
        is_torch = type(owner).__module__.split(".")[0] == "torch"
        if out is None:
            if not is_torch:
                raise ValueError("impute(): out=None allocates the result, which the library does only for torch tensors; "
                                 "pass out= (out=data fills in place)")
            import torch
            res = torch.empty_like(owner)
            return res.data_ptr(), res
        if out is data:
            if is_torch and (owner.dtype != data.dtype or not data.is_contiguous()):
                raise ValueError("impute(): out=data needs contiguous float32 rows; these had to be converted, so a fill in "
                                 "place would not reach them")
            if not is_torch and data.__cuda_array_interface__["data"][1]:
                raise ValueError("impute(): out is read-only")
            return ptr, data
        if type(out).__module__.split(".")[0] == "torch" and getattr(out, "is_cuda", False):
            import torch
            if out.dtype != torch.float32 or not out.is_contiguous():
                raise ValueError("impute(): out must be a C-contiguous float32 array, got %s%s" % (
                    out.dtype, "" if out.is_contiguous() else ", not contiguous"))
            if tuple(out.shape) != (n, d):
                raise ValueError("impute(): out has shape %r, the rows %r" % (tuple(out.shape), (n, d)))
            if out.device.index != eng.device:
                raise ValueError('impute(): out lives on cuda:%d, the engine on cuda:%d' % (out.device.index, eng.device))
            torch.cuda.current_stream(out.device).synchronize()
            out_ptr = out.data_ptr()
        else:
            cai = getattr(out, "__cuda_array_interface__", None)
            if cai is None:
                raise ValueError("impute(): out must be an array in device memory (a torch CUDA tensor or a "
                                 "__cuda_array_interface__ object)")
            if cai["typestr"] != "<f4" or cai.get("strides") is not None:
                raise ValueError("impute(): out must be a C-contiguous float32 array")
            if tuple(cai["shape"]) != (n, d):
                raise ValueError("impute(): out has shape %r, the rows %r" % (tuple(cai["shape"]), (n, d)))
            if cai["data"][1]:
                raise ValueError("impute(): out is read-only")
            eng.sync_producer(cai.get("stream"))
            out_ptr = int(cai["data"][0])
        nbytes = n * d * 4
        if out_ptr != ptr and out_ptr < ptr + nbytes and ptr < out_ptr + nbytes:
            raise ValueError("impute(): out overlaps the rows without being the same array")
        return out_ptr, out

    def impute(self, data, *, out=None, return_ids=False):
        """The samples with every NaN replaced by the value their best matching unit holds for that feature; needs
        ``missing='nan'``.  The unit is the one ``predict`` names (the search over the row's observed features); observed
        values come back bit for bit (``-0.0``, ``inf`` and denormals as they are), the filled ones are the float32 codebook
        values bit for bit; a row with nothing observed becomes unit 0's vector, a complete row is returned as it is.  If the
        codebook itself holds a NaN (``_weights`` set by hand), that NaN is copied.  Train on ``[X | y]``, query with
        ``y = NaN`` and read ``y`` off the result: the map as a predictor.

        Host rows (array-like; a 1-D input is one sample and returns 1-D): a new float32 array of the input's shape, in
        ``n_parallel`` chunks; the input is never modified and ``out`` must be ``None``.  Rows in HBM (a torch CUDA tensor or a
        ``__cuda_array_interface__`` object) are searched and filled where they are, whole: ``out=None`` returns a new tensor
        on the same device (torch only: the library allocates nothing else that it hands to a caller), ``out=data`` fills in
        place and returns ``data``, any other ``out`` must be a writable C-contiguous float32 device array of the same shape
        on the engine's device that does not partly overlap the rows.  ``return_ids=True`` returns ``(rows, ids)``, ids int64
        and raveled as in ``predict``."""
        if getattr(self, '_missing', None) != 'nan':
            raise ValueError("impute() needs missing='nan': without it a NaN is a value like any other, and there is nothing to fill")
        if out is not None and not _is_device_array(data):
            raise ValueError("impute(): out is for rows in device memory; host rows return a new array")
        q = self._device_query(data)
        if q is not None:
            eng, ptr, n, owner = q
            out_ptr, res = self._impute_out(data, owner, ptr, n, out, eng)
            ids = eng.impute_device(ptr, n, out_ptr) if n else np.zeros(0, np.int32)
            return (res, ids.astype(np.int64)) if return_ids else res
        if out is not None:
            raise ValueError("impute(): out needs 2-dimensional rows in device memory")
        data = _host_rows(data, self._engine)
        one = data.ndim == 1
        if one:
            data = data[None, :]
        if len(data):
            self._check_input_len(data)
        eng = self._upload_weights()
        parts = [eng.impute(data[s:s + self._n_parallel]) for s in range(0, len(data), self._n_parallel)]
        rows = np.concatenate([p[0] for p in parts]) if parts else np.empty(data.shape, dtype=np.float32)
        ids = np.concatenate([p[1] for p in parts]).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
        if one:
            rows = rows[0]
        return (rows, ids) if return_ids else rows

    def unit_statistics(self, data):
        """Per-unit statistics of the samples' distances to their best matching units, a ``UnitStatistics`` of ``(x, y)``
        arrays: ``hits`` (samples the unit wins), ``sum`` and ``sumsq`` of their distances (float64), ``max`` (float32), with
        ``mean`` -- the quantization-error map -- and ``std`` derived.  Computed on the device without floating-point
        atomics: the same rows give the same bits.  Host rows go in ``n_parallel`` chunks whose results are added on the
        host in chunk order (float64; ``max`` by ``np.maximum``)."""
        eng, q, data = self._diag_query(data)
        X, Y = self._weights.shape[:2]
        hits, tot = np.zeros(X * Y, dtype=np.int64), np.zeros(X * Y, dtype=np.float64)
        sq, mx = np.zeros(X * Y, dtype=np.float64), np.zeros(X * Y, dtype=np.float32)
        if q is not None:
            parts = [eng.unit_stats_device(q[1], q[2])] if q[2] else []
        else:
            parts = (eng.unit_stats(data[s:s + self._n_parallel]) for s in range(0, len(data), self._n_parallel))
        for c, s, s2, m in parts:
            hits += c
            tot += s
            sq += s2
            mx = np.maximum(mx, m)
        return UnitStatistics(hits.reshape(X, Y), tot.reshape(X, Y), sq.reshape(X, Y), mx.reshape(X, Y))

    def _density_pivot(self):
        """The midrange of the codebook the engine holds, float32 (D,): the point the density scan centres rows and units on."""
        w = np.asarray(self._weights, dtype=np.float32).reshape(-1, self._input_len).astype(np.float64)
        return ((w.min(axis=0) + w.max(axis=0)) / 2).astype(np.float32)

    def density_map(self, data, radius):
        """The data density per unit, Ultsch's P-matrix: int64 ``(x, y)``, element ``[i, j]`` the number of samples within
        ``radius`` (Euclidean, inclusive) of unit ``(i, j)``'s weight vector.  A sequence of 1 to 8 radii gives
        ``(len(radius), x, y)`` from ONE pass over the data.  Unlike every other per-unit map this does not follow from the
        samples' best matching units: it is a full samples x units scan, counted on the device in float32 without ever
        writing the distance matrix.  Rows and units are centred on the midrange of the codebook first (distances are
        translation invariant; the GEMM form of the distance cancels on un-centred data), so a sample whose distance is within
        a few parts in a thousand of the radius may fall on either side; a sample holding a NaN or an infinity is counted
        nowhere.  Rows in HBM are counted where they are, whole; host rows in ``n_parallel`` chunks whose counts are added.
        The counts of shards or ranks add as well.

        Picking a radius: pass several in one call; Ultsch's Pareto radius is the one at which the median over the units of
        ``P / n_samples`` is about 0.2.  ``ustar_map`` combines the result with the U-matrix.
        Not defined with ``missing='nan'``."""
        from .engine import check_radii
        self._refuse_missing('density_map')
        scalar = np.ndim(radius) == 0
        radii = check_radii(radius)
        eng, q, data = self._diag_query(data)
        X, Y = self._weights.shape[:2]
        pivot = self._density_pivot()
        counts = np.zeros((len(radii), X * Y), dtype=np.int64)
        if q is not None:
            if q[2]:
                counts += eng.unit_density_device(q[1], q[2], pivot, radii)
        else:
            for s in range(0, len(data), self._n_parallel):
                counts += eng.unit_density(data[s:s + self._n_parallel], pivot, radii)
        return counts[0].reshape(X, Y) if scalar else counts.reshape(len(radii), X, Y)

    def ustar_map(self, data, radius):
        """The U*-matrix (Ultsch): the U-matrix scaled down where the data is dense, ``U * ((P - mean P) / (mean P - max P) + 1)``
        with ``U = distance_map()`` and ``P = density_map(data, radius)`` (one radius) -- ``U`` where the density is average, 0
        where it is highest, above ``U`` where it is sparse; ``U`` unchanged where the density is flat.  It tells "far apart
        because there is a gap in the data" from "far apart inside a dense cluster".  float64 ``(x, y)``."""
        self._refuse_missing('ustar_map')
        if np.ndim(radius) != 0:
            raise ValueError("ustar_map() takes one radius, got %r" % (radius,))
        p = self.density_map(data, radius)
        return _ustar(self.distance_map(), p)

    def _topk_query(self, what, data, k):
        """(engine, device query or None, host rows or None, k) of a ranked-list query, refused by name where it is not defined."""
        from .engine import check_topk
        self._refuse_missing(what)
        if self._activation_distance_name not in ('euclidean', 'euclidean_no_opt', 'cosine'):
            raise NotImplementedError("%s() ranks the units by the GEMM-form distances only (euclidean, euclidean_no_opt, cosine); "
                                      "'%s' is a fused distance+argmin kernel here" % (what, self._activation_distance_name))
        k = check_topk(k)
        X, Y = self._weights.shape[:2]
        if k > X * Y:
            raise ValueError("%s(): k = %d exceeds the map's %d units" % (what, k, X * Y))
        eng, q, data = self._diag_query(data)
        return eng, q, data, k

    def nearest_units(self, data, k, *, return_distance=True):
        """The k nearest units of every sample: ``ids`` int64 ``(n, k)``, raveled as in ``predict``, and ``dist`` float32
        ``(n, k)`` (``return_distance=False``: ``ids`` alone).  Row n lists the k units with the smallest activation distance to
        sample n under ``activation_distance`` ('euclidean', 'euclidean_no_opt' or 'cosine'), nearest first, equal distances to the
        lower unit id -- the ranking ``activate(data)`` and a stable argsort would give, found on the device without ever
        writing the ``(n, K)`` matrix.  The search is float32 whatever ``precision`` is; with 'f32' and 'exact' column 0 is
        ``predict(data)``.  ``dist[n, j]`` is the Euclidean distance of the sample to unit ``ids[n, j]``, formed from the
        differences as in ``quantization_distances`` -- always Euclidean, and not what orders the list: with a Euclidean
        activation it ascends along a row only up to rounding, with 'cosine' it need not ascend at all.  A sample holding a NaN
        or an infinity has no distance below infinity to any unit under the Euclidean activations: its row is ``-1`` / NaN, as is
        every slot beyond the units that have one.  ``1 <= k <= 8`` and ``k <= x * y``.  Rows in HBM are searched where they
        are; host rows in ``n_parallel`` chunks.  Not defined with ``missing='nan'``."""
        eng, q, data, k = self._topk_query('nearest_units', data, k)
        if q is not None:
            parts = [eng.bmu_topk_device(q[1], q[2], k, score=False, dist=return_distance)] if q[2] else []
        else:
            parts = [eng.bmu_topk(data[s:s + self._n_parallel], k, score=False, dist=return_distance)
                     for s in range(0, len(data), self._n_parallel)]
        ids = np.concatenate([p[0] for p in parts]).astype(np.int64) if parts else np.zeros((0, k), dtype=np.int64)
        if not return_distance:
            return ids
        return ids, (np.concatenate([p[2] for p in parts]) if parts else np.zeros((0, k), dtype=np.float32))

    def rank_hits(self, data, k):
        """int64 ``(k, x, y)``: element ``[j, a, b]`` is the number of samples whose j-th nearest unit (``nearest_units``' column
        j) is unit ``(a, b)``, counted on the device -- the ranked lists are never copied out.  With ``precision`` 'f32' or
        'exact' ``rank_hits(data, 1)[0]`` equals ``activation_response(data)``.  The counts of chunks, shards and ranks add."""
        return self._rank_hits('rank_hits', data, k)

    def _rank_hits(self, what, data, k):
        eng, q, data, k = self._topk_query(what, data, k)
        X, Y = self._weights.shape[:2]
        counts = np.zeros((k, X * Y), dtype=np.int64)
        if q is not None:
            if q[2]:
                counts += eng.unit_rank_counts_device(q[1], q[2], k)
        else:
            for s in range(0, len(data), self._n_parallel):
                counts += eng.unit_rank_counts(data[s:s + self._n_parallel], k)
        return counts.reshape(k, X, Y)

    def smoothed_hits(self, data, s):
        """Pampalk's smoothed data histogram, float64 ``(x, y)``: every sample gives ``s - j`` points to its j-th nearest unit
        (j = 0 .. s-1), divided by ``s (s + 1) / 2`` -- a hit histogram in which a sample votes for its ``s`` nearest units
        instead of one, which shows the cluster structure of maps with more units than a plain hit count can fill.  ``s = 1`` is
        ``activation_response``.  Formed on the host from ``rank_hits(data, s)``; it sums to the number of samples whose lists
        are full."""
        return _sdh(self._rank_hits('smoothed_hits', data, s))

    def _column_query(self, eng, col, what, dtype_name, typestr, host):
        """(pointer, owner) of the labels or values that go with device rows: a device array is read where it is (its
        producer waited for), the checked host array `host` is copied next to the rows."""
        if host is not None:
            owner = _to_device(host, eng.device)
            return owner.data_ptr(), owner
        ptr, _shape, dev_index, owner, stream = _device_column(col, dtype_name, typestr)
        if dev_index is not None and dev_index != eng.device:
            raise ValueError('device %s live on cuda:%d, the engine on cuda:%d' % (what, dev_index, eng.device))
        if stream != "done":
            eng.sync_producer(stream)
        return ptr, owner

    def label_counts(self, data, labels, n_classes=None):
        """The label map as an array: int64 ``(x, y, n_classes)``, element ``[i, j, c]`` the number of samples whose best
        matching unit is ``(i, j)`` (the units of ``predict`` / ``labels_map``: the configured distance) and whose label is
        ``c`` -- ``labels_map``'s Counters, counted on the device.  ``labels`` holds one integer class code per sample: a
        host array-like, or for rows in HBM a 1-D device int32 tensor next to them (a host array is copied there); any
        negative code means unlabelled and is counted nowhere.  ``n_classes`` defaults to ``max(labels) + 1`` and is required
        for device labels (codes ``>= n_classes`` there are counted nowhere); host codes ``>= n_classes`` raise
        ``ValueError``.  Rows in HBM go whole; host rows in ``n_parallel`` chunks whose counts are added on the host.  No
        sample weights, no neighbourhood smoothing, no cross-rank reduction: each rank reports its own rows, and the counts
        add."""
        eng, q, data = self._diag_query(data)
        X, Y = self._weights.shape[:2]
        n = q[2] if q is not None else len(data)
        lab32 = None
        if n_classes is not None:
            if isinstance(n_classes, (bool, np.bool_)) or int(n_classes) != n_classes or not 1 <= n_classes <= 4096:
                raise ValueError('n_classes must be an integer between 1 and 4096, got %r' % (n_classes,))
            n_classes = int(n_classes)
        if _is_device_array(labels):
            if q is None:
                raise ValueError('labels in device memory need data in device memory')
            if n_classes is None:
                raise ValueError('n_classes is required for labels in device memory')
            if tuple(_n_shape(labels)) != (n,):
                raise ValueError('data and labels must have the same length.')
        else:
            lab = np.asarray(labels)
            if lab.ndim != 1 or len(lab) != n:
                raise ValueError('data and labels must have the same length.')
            if len(lab) and (lab.dtype == np.bool_ or not np.issubdtype(lab.dtype, np.integer)):
                raise ValueError('labels must be integer class codes, got dtype %s' % (lab.dtype,))
            top = int(lab.max()) if len(lab) else -1
            if n_classes is None:
                if top < 0:
                    raise ValueError('n_classes cannot be inferred: no sample is labelled')
                n_classes = top + 1
                if n_classes > 4096:
                    raise ValueError('labels hold codes up to %d: at most 4096 classes' % top)
            if top >= n_classes:
                raise ValueError('labels must be < n_classes = %d, got %d' % (n_classes, top))
            lab32 = np.where(lab < 0, -1, lab).astype(np.int32) if len(lab) else np.zeros(0, np.int32)
        counts = np.zeros((X * Y, n_classes), dtype=np.int64)
        if q is not None:
            if n:
                ptr, _owner = self._column_query(eng, labels, 'labels', 'int32', '<i4', lab32)
                counts += eng.label_counts_device(q[1], ptr, n, n_classes)
        else:
            for s in range(0, n, self._n_parallel):
                counts += eng.label_counts(data[s:s + self._n_parallel], lab32[s:s + self._n_parallel], n_classes)
        return counts.reshape(X, Y, n_classes)

    def unit_means(self, data, values):
        """Per-unit statistics of ``values`` -- one or more columns of numbers the map was not trained on, ``(n,)`` or
        ``(n, n_cols)`` float32 -- over the samples each unit wins (the units of ``predict``): a ``UnitMeans`` of
        ``(x, y, n_cols)`` arrays ``count``, ``sum``, ``sumsq`` (float64 sums) with ``mean`` -- the component planes -- and
        ``std`` derived.  A NaN value is "not observed" for its column only, whatever ``missing`` is; +-Inf is a value.  For
        rows in HBM ``values`` is a device float32 tensor next to them (a host array is copied there).  Computed on the
        device without atomics: the same rows give the same bits.  Rows in HBM go whole; host rows in ``n_parallel`` chunks
        whose results are added on the host in chunk order (float64).  No sample weights, no neighbourhood smoothing, no
        cross-rank reduction: each rank reports its own rows, and the three raw arrays add."""
        eng, q, data = self._diag_query(data)
        X, Y = self._weights.shape[:2]
        n = q[2] if q is not None else len(data)
        val = None
        if _is_device_array(values):
            if q is None:
                raise ValueError('values in device memory need data in device memory')
            shape = tuple(_n_shape(values))
        else:
            val = np.asarray(values)
            if val.dtype == np.bool_ or not (np.issubdtype(val.dtype, np.integer) or np.issubdtype(val.dtype, np.floating)):
                raise ValueError('values must have a real dtype, got %s' % (val.dtype,))
            val = np.ascontiguousarray(val, dtype=np.float32)
            if val.ndim == 1:
                val = val[:, None]
            shape = val.shape
        if len(shape) not in (1, 2) or shape[0] != n:
            raise ValueError('data and values must have the same length.')
        n_cols = shape[1] if len(shape) == 2 else 1
        if not 1 <= n_cols <= 4096:
            raise ValueError('values must have between 1 and 4096 columns, got %d' % n_cols)
        count = np.zeros((X * Y, n_cols), dtype=np.int64)
        tot, sq = np.zeros((X * Y, n_cols), dtype=np.float64), np.zeros((X * Y, n_cols), dtype=np.float64)
        if q is not None:
            parts = []
            if n:
                ptr, _owner = self._column_query(eng, values, 'values', 'float32', '<f4', val)
                parts = [eng.value_sums_device(q[1], ptr, n, n_cols)]
        else:
            parts = (eng.value_sums(data[s:s + self._n_parallel], val[s:s + self._n_parallel]) for s in range(0, n, self._n_parallel))
        for c, s, s2 in parts:
            count += c
            tot += s
            sq += s2
        return UnitMeans(count.reshape(X, Y, n_cols), tot.reshape(X, Y, n_cols), sq.reshape(X, Y, n_cols))

    def classify(self, data, counts, default=None):
        """Class code (int64) of every sample from a label map ``counts`` (``label_counts`` of labelled samples,
        ``(x, y, n_classes)``): the most frequent class of the sample's best matching unit, the lowest code on a tie.  A unit
        without a labelled sample gives ``default``; ``None`` means the class with the largest total over the map (the
        lowest code on a tie).  The rule of MiniSom's classification example without its per-sample ``winner`` loop; the
        map is taken as it is (no smoothing over neighbouring units)."""
        X, Y = self._weights.shape[:2]
        counts = np.asarray(counts)
        if counts.ndim != 3 or counts.shape[:2] != (X, Y) or counts.shape[2] < 1:
            raise ValueError('counts must be (%d, %d, n_classes), got %r' % (X, Y, counts.shape))
        flat = counts.reshape(X * Y, -1)
        if default is None:
            default = int(np.argmax(flat.sum(axis=0)))
        per_unit = np.where(flat.sum(axis=1) > 0, np.argmax(flat, axis=1), default).astype(np.int64)
        if self._device_query(data) is None:
            data = _host_rows(data, self._engine)
            if data.ndim == 1:
                data = data[None, :]
            if len(data):
                self._check_input_len(data)
        return per_unit[self.predict(data)]

    def topographic_error(self, data):
        """Share of samples whose best and second-best matching units are not adjacent on the map
        (xpysom.py:709-746, rectangular branch: |di| > 1 or |dj| > 1).  The reference sorts the whole
        (n, K) distance matrix; here a fused top-2 variant of the BMU kernel returns the pair."""
        self._refuse_missing('topographic_error')
        # rows in HBM are searched where they are, whole (som_bmu_top2_device); host rows in n_parallel chunks
        q = self._device_query(data)                        # (checks the feature count of device rows itself)
        if q is None:
            self._check_input_len(data)
        if np.prod(self._weights.shape) == 1:
            warn('The topographic error is not defined for a 1-by-1 map.')
            return np.nan
        if q is None:
            data = _host_rows(data, self._engine)
        n_rows = q[2] if q is not None else len(data)
        if self._weights.shape[0] * self._weights.shape[1] == 1 and n_rows:
            # one unit, input_len > 1: argsort(...)[:, :2] holds one column and its diff none -- the reference's mean over
            # an empty axis is NaN (rectangular), its norm over one is 0 (hexagonal: 0 > 1.5 never)
            return 0.0 if self.topology == 'hexagonal' else float('nan')
        eng = q[0] if q is not None else self._upload_weights()   # (_device_query has uploaded the codebook)
        Y = self._weights.shape[1]
        bad, n = 0, 0
        if q is not None:
            pairs = [eng.bmu_top2_device(q[1], n_rows)] if n_rows else []
        else:
            pairs = (eng.bmu_top2(data[s:s + self._n_parallel]) for s in range(0, n_rows, self._n_parallel))
        for b1, b2 in pairs:
            bad += int((~units_adjacent(b1, b2, self._weights.shape[0], Y, self.topology)).sum())
            n += len(b1)
        return bad / n if n else float('nan')

    def predict(self, data):
        """Raveled BMU index of every sample (xpysom.py:608-617), batched."""
        return self._ids_of(data).astype(np.int64)

    def _rows_by_unit(self, data):
        """BMU ids of `data` grouped: yields ((i, j), row indices in data order), units in order of first win --
        one batched BMU call and one stable sort instead of a winner() call per sample."""
        ids = self._ids_of(data).astype(np.int64)
        if not len(ids):
            return
        order = np.argsort(ids, kind='stable')
        cuts = np.flatnonzero(np.diff(ids[order])) + 1
        groups = np.split(order, cuts)
        Y = self._weights.shape[1]
        for rows in sorted(groups, key=lambda r: r[0]):
            i, j = np.divmod(ids[rows[0]], Y)
            yield (i, j), rows

    def activation_response(self, data):
        """Matrix where element i,j is the number of times neuron i,j won (xpysom.py:819-829)."""
        if self._device_query(data) is None:
            data = _host_rows(data, self._engine)
            self._check_input_len(data)
        X, Y = self._weights.shape[:2]
        return np.bincount(self._ids_of(data), minlength=X * Y).astype(float).reshape(X, Y)

    def win_map(self, data):
        """Dictionary wm where wm[(i,j)] lists the patterns mapped to i,j (xpysom.py:831-840)."""
        self._check_input_len(data)
        winmap = defaultdict(list)
        host = data if hasattr(data, '__getitem__') and _device_rows(data) is None else _host_rows(data, self._engine)
        for unit, rows in self._rows_by_unit(host):
            winmap[unit] = [host[n] for n in rows]
        return winmap

    def labels_map(self, data, labels):
        """Dictionary wm where wm[(i,j)] counts the labels mapped to i,j (xpysom.py:842-865)."""
        self._check_input_len(data)
        if not len(data) == len(labels):
            raise ValueError('data and labels must have the same length.')
        winmap = defaultdict(list)
        for unit, rows in self._rows_by_unit(data):
            winmap[unit] = Counter(labels[n] for n in rows)
        return winmap

    # ------------------------------------------------------------------ host-side initialisers
    def _init_device_rows(self, dev, what):
        """(pointer, n_rows, engine, owner) of device rows handed to an initialiser -- `dev`: what ``_device_rows`` returned for
        them, resolved ONCE per call (each resolution waits for torch's stream and, for a tensor that is not contiguous float32,
        makes a converted copy) --, checked and waited for.  The caller holds `owner` for as long as the pointer is in use: for a
        converted tensor it is the only reference to the copy the pointer points into."""
        ptr, n, d, dev_index, owner, stream = dev
        if d != self._input_len:
            raise ValueError('Received %d features, expected %d.' % (d, self._input_len))
        if self._input_len > 2048 and what != 'random_weights_init':
            raise ValueError('%s: the device moments take up to 2048 features, got %d' % (what, self._input_len))
        eng = self._engine()
        if dev_index is not None and dev_index != eng.device:
            raise ValueError('device data lives on cuda:%d, the engine on cuda:%d' % (dev_index, eng.device))
        if stream != "done":
            eng.sync_producer(stream)
        return ptr, n, eng, owner

    def _row_moments(self, data, weights=None, what='linear_weights_init', grouped=False):
        """``(wsum, mean, M)`` in float64 from the device moments (include/somhip.h, som_row_moments): ``wsum = sum w``, the weighted
        mean, and ``M = sum w (x - mean)(x - mean)^T`` -- divide by ``wsum`` or ``n - 1`` for a covariance.  Two passes: the sums
        give the mean, the Gram matrix is taken about ``float32(mean)`` and shifted exactly in float64, so the pivot's rounding costs
        nothing.  Device rows in one call per pass; host rows in ``n_parallel`` chunks, every chunk's result added in chunk order.
        ``grouped``: under a process group the rows (and weights) are cut as ``train`` cuts them and both passes are all-reduced, so
        every rank returns the same bits.  ``weights``: what ``_check_sample_weight`` returned, or None."""
        rank, world = _dist.dist_info() if grouped else (0, 1)
        if world > 1 and not self._sharded_input:
            shard = getattr(self, '_shard', 'contiguous')
            data = _dist.shard_rows(data, rank, world, shard)
            if weights is not None:
                weights = _dist.shard_rows(weights, rank, world, shard)
        dev = _device_rows(data)                         # (once, after the cut: see _init_device_rows)
        if dev is not None:
            # owner / wowner: whatever owns the rows and the weights behind ptr / wptr, held by `passes` until both passes are done
            ptr, n, eng, owner = self._init_device_rows(dev, what)
            wptr = wowner = None
            if weights is not None:
                if not _is_device_array(weights):        # host weights beside device rows: they join them on the device
                    weights = _to_device(np.ascontiguousarray(weights, dtype=np.float32), eng.device)
                wptr, wdev, wowner, wstream = _device_weights(weights)
                if wdev is not None and wdev != eng.device:
                    raise ValueError('sample_weight lives on cuda:%d, the engine on cuda:%d' % (wdev, eng.device))
                if wstream != "done":
                    eng.sync_producer(wstream)

            def passes(pivot, gram, _keepalive=(owner, wowner)):
                yield eng.row_moments_device(ptr, n, wptr, pivot, gram)
        else:
            data = np.asarray(data, dtype=np.float32)
            if data.ndim != 2:
                raise ValueError('data must be 2-dimensional (n_samples, input_len)')
            if self._input_len > 2048:
                raise ValueError('%s: the device moments take up to 2048 features, got %d' % (what, self._input_len))
            eng = self._engine()
            step = max(1, int(self._n_parallel))

            def passes(pivot, gram):
                for lo in range(0, len(data), step):
                    yield eng.row_moments(data[lo:lo + step], None if weights is None else weights[lo:lo + step], pivot, gram)
        D = self._input_len
        wsum, s1 = 0.0, np.zeros(D)
        for w_, s_, _ in passes(None, False):
            wsum += w_
            s1 += s_
        wsum, s1 = _dist.allreduce_moments(eng, world, wsum, s1)
        if not (np.isfinite(wsum) and np.isfinite(s1).all()):
            raise ValueError(_nan_init_message(what))
        if not wsum > 0:
            raise ValueError('%s: the sample weights sum to 0' % what)
        pivot = (s1 / wsum).astype(np.float32)
        wsum, s1, G = 0.0, np.zeros(D), np.zeros((D, D))
        for w_, s_, g_ in passes(pivot, True):
            wsum += w_
            s1 += s_
            G += g_
        wsum, s1, G = _dist.allreduce_moments(eng, world, wsum, s1, G)
        if not (np.isfinite(s1).all() and np.isfinite(G).all()):
            raise ValueError(_nan_init_message(what))
        return wsum, pivot.astype(np.float64) + s1 / wsum, G - np.outer(s1, s1) / wsum

    def random_weights_init(self, data):
        """Initializes the weights picking random samples from data (xpysom.py:749-759).  Rows that live in HBM are picked by the
        same stream of indices and gathered on the device: the host path's codebook for the same seed, bit for bit."""
        x, y, _ = self._weights.shape
        dev = _device_rows(data)
        if dev is not None:
            ptr, n, eng, owner = self._init_device_rows(dev, 'random_weights_init')     # (owner: held until the gather is done)
            if getattr(self, '_missing', None) is not None:
                # as on the host path: any NaN in the data is refused BEFORE an index is drawn, so a refusal leaves the generator alone
                import torch
                if bool(torch.isnan(torch.as_tensor(owner, device=torch.device("cuda", eng.device))).any()):
                    raise ValueError(_nan_init_message('random_weights_init'))
            # (one call draws the stream of x * y scalar calls: tests/test_init_cpu.py pins it)
            rows = eng.gather_rows_device(ptr, n, self._random_generator.randint(n, size=x * y))
            del owner
            self._weights[...] = rows.reshape(x, y, -1)
            return
        self._check_input_len(data)
        self._refuse_nan_init('random_weights_init', data)
        for i in range(x):
            for j in range(y):
                self._weights[i, j] = data[self._random_generator.randint(len(data))]

    def pca_weights_init(self, data):
        """Initializes the weights to span the first two principal components (xpysom.py:762-785).  Rows that live in HBM: the
        covariance (divisor n - 1, as ``np.cov``) comes from the device moments, then the same ``eig`` and formula."""
        if self._input_len == 1:
            raise ValueError('The data needs at least 2 features for pca initialization')
        on_device = _is_device_array(data)
        if not on_device:
            self._check_input_len(data)
            self._refuse_nan_init('pca_weights_init', data)
        elif _n_rows(data) < 2:                          # (np.cov's divisor n - 1)
            raise ValueError('pca_weights_init: the data needs at least 2 rows, got %d' % _n_rows(data))
        if len(self._neigx) == 1 or len(self._neigy) == 1:
            warn('PCA initialization inappropriate:One of the dimensions of the map is 1.')
        if on_device:
            wsum, _, M = self._row_moments(data, None, 'pca_weights_init')
            cov = M / (wsum - 1.0)
        else:
            cov = np.cov(np.transpose(data))
        self._weights[...] = _pca_codebook(cov, len(self._neigx), len(self._neigy))

    def linear_weights_init(self, data, *, sample_weight=None):
        """Places the map in the data (not in the reference; the SOM Toolbox's ``lininit``): the weighted mean plus the two leading
        principal axes scaled by their standard deviations -- ``_linear_codebook`` of the weighted moments with divisor ``sum w``, so
        an integer weight is the row repeated.  Host rows or rows that live in HBM; ``sample_weight`` as ``train`` takes it.  The
        moments are computed on the device either way (``_row_moments``).  Under a process group the rows are cut as ``train`` cuts
        them and every rank ends with the same codebook."""
        if self._input_len == 1:
            raise ValueError('The data needs at least 2 features for linear initialization')
        on_device = _is_device_array(data)
        if not on_device:
            data = np.asarray(data, dtype=np.float32)
            if data.ndim != 2:
                raise ValueError('data must be 2-dimensional (n_samples, input_len)')
            if len(data) > 0:
                self._check_input_len(data)
        weights = None
        if sample_weight is not None:
            weights = _check_sample_weight(sample_weight, _n_rows(data), on_device)
        wsum, mean, M = self._row_moments(data, weights, 'linear_weights_init', grouped=True)
        x, y, _ = self._weights.shape
        self._weights = _linear_codebook(wsum, mean, M / wsum, x, y).astype(np.float32)

    # ------------------------------------------------------------------ pickling (xpysom.py:868-892)
    def __getstate__(self):
        state = self.__dict__.copy()
        state['_engine_obj'] = None          # device handle: rebuilt lazily from (config, weights)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault('_missing', None)        # (a pickle from before the keyword)
        self.__dict__.setdefault('history', [])
