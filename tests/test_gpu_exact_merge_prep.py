"""Exact mode, euclidean, up to 128 features: the FUSED MERGE (exact_merge_prep_kernel: merged codebook, patch-order copy,
|w|^2, screen norms and their maximum, float32 stage image, the plan's centroids -- one launch) against the separate
kernels it replaces (SOM_FUSE_MERGE=0: merge_kernel, row_sq_f32_kernel, exact_copy_wsq_kernel, prep_w_f32_res_kernel,
exact_centroids_kernel).

Every case runs the same seeded epochs on two fresh engines, one per path, and asserts epoch by epoch: the codebook
bitwise, the epoch's BMU ids, exact_skip_stats() and exact_stats() (centroids, radii and images feed only the plan: the
same executed-block counts are the observable proof that they did not move), and a hash of every operand buffer after
the BMU launch has prepared the 16-bit images (som_debug_operand_crc).

Shapes: the smallest that reach each branch.  SOM_EXACT_SKIP=2 forces the plan on every map of two groups
or more (and takes the measured-cost decisions out of the policy: the two engines then plan alike by construction)."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from xpysom_dask_amd.synthetic import gaussian_blobs

pytestmark = pytest.mark.gpu

N_ROWS = 4096
OPERANDS = ("Wst", "Wst_lo", "Wfst", "wsq_image_order", "wn", "wmax2", "centroids", "W_image_order")


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _engine(fused, x, y, d, skip, **kw):
    from xpysom_dask_amd.engine import HipEngine
    # (the library reads both switches in som_create; SOM_FUSE_MERGE only under SOM_TEST_HOOKS=1, which conftest sets)
    with _env(SOM_FUSE_MERGE="1" if fused else "0", SOM_EXACT_SKIP=str(skip)):
        return HipEngine(x, y, d, precision="exact", **kw)


def _crcs(eng):
    out = []
    for which in range(len(OPERANDS)):
        v = C.c_uint64()
        eng._check(eng._lib.som_debug_operand_crc(eng._h, which, C.byref(v)))
        out.append(v.value)
    return out


def _codebook(x, y, d, seed):
    return np.random.default_rng(seed).normal(0.0, 2.0, size=(x * y, d)).astype(np.float32)


def _run(fused, x, y, d, *, rows, w0, sigmas, skip=2, forced_first=False, reset_after=None, **kw):
    """The record of one engine: per step (BMU ids, operand hashes after the launch, codebook after the merge, the counters,
    did the step's launch run under a plan over the resident rows)."""
    eng = _engine(fused, x, y, d, skip, **kw)
    rec = []
    planned = 0
    try:
        eng.set_weights(w0)
        eng.set_data(rows)
        for e, sigma in enumerate(sigmas):
            if forced_first and e == 0:
                # (a merge before any BMU launch: the ids are given)
                eng.epoch_accumulate_forced(np.arange(len(rows), dtype=np.int32) % (x * y), sigma, 0.5, 1)
            else:
                eng.epoch_accumulate(sigma, 0.5, 1)
            _, _, bmu = eng.epoch_fetch()
            # (the forced epoch launched no search: nothing has prepared the operands yet)
            crc = _crcs(eng) if not (forced_first and e == 0) else [0] * len(OPERANDS)
            eng.epoch_merge()
            was, planned = planned, eng.exact_resident_stats()[0]
            rec.append((bmu, crc, eng.get_weights(), eng.exact_skip_stats(), eng.exact_stats(), planned > was))
            if reset_after == e:
                # set_weights between two epochs, then a query before the next merge: the dirty-flag fallbacks
                eng.set_weights(w0[::-1].copy())
                q = eng.bmu(rows[:300])
                rec.append((q, _crcs(eng), eng.get_weights(), eng.exact_skip_stats(), eng.exact_stats(), False))
        # the operands of the LAST merged codebook: a query prepares them
        q = eng.bmu(rows[:300])
        rec.append((q, _crcs(eng), eng.get_weights(), eng.exact_skip_stats(), eng.exact_stats(), False))
    finally:
        eng.close()
    return rec


def _compare(x, y, d, **kw):
    ref = _run(False, x, y, d, **kw)
    got = _run(True, x, y, d, **kw)
    assert len(ref) == len(got)
    for e, (r, g) in enumerate(zip(ref, got)):
        assert np.array_equal(r[0], g[0]), "step %d: BMU ids differ in %d rows" % (e, int((r[0] != g[0]).sum()))
        assert r[2].view(np.uint32).tobytes() == g[2].view(np.uint32).tobytes(), "step %d: the codebooks differ" % e
        assert r[3] == g[3], "step %d: exact_skip_stats %r != %r" % (e, g[3], r[3])
        assert r[4] == g[4], "step %d: exact_stats %r != %r" % (e, g[4], r[4])
        assert r[5] == g[5], "step %d: one engine planned, the other did not" % e
        # (the centroid buffers are rewritten by launches that plan: only there do the separate kernels leave current ones)
        bad = [OPERANDS[i] for i in range(len(OPERANDS)) if r[1][i] != g[1][i] and (OPERANDS[i] != "centroids" or r[5])]
        assert not bad, "step %d: operand buffers differ: %s" % (e, ", ".join(bad))
    return ref


SIGMAS = (6.0, 4.0, 3.0, 2.0)


# a: the headline's instance (four 32-feature steps, whole groups);  b: the other instances;  c: input_len no multiple of 4 / 8
@pytest.mark.parametrize("d", [128, 32, 64, 96, 20, 100])
def test_fused_merge_features(d):
    rows = gaussian_blobs(N_ROWS, d, seed=11)
    ref = _compare(64, 64, d, rows=rows, w0=_codebook(64, 64, d, 5), sigmas=SIGMAS)
    run, total = ref[-1][3]
    assert 0 < run < total                                  # (the plan engaged: the centroids were read)


# d: K no multiple of 64 or of 16 -- a partial group, a partial 16-unit tile, level-2 slots without units (10 x 10: two
#    groups, no patch order)
@pytest.mark.parametrize("x,y", [(10, 10), (67, 61)])
def test_fused_merge_partial_groups(x, y):
    rows = gaussian_blobs(N_ROWS, 128, seed=12)
    _compare(x, y, 128, rows=rows, w0=_codebook(x, y, 128, 6), sigmas=(3.0, 2.0, 1.5) if x == 10 else SIGMAS)


# e: units no row reaches (den == 0) keep their old row in W, Wp and every image
@pytest.mark.parametrize("neigh", [dict(neighborhood="bubble"), dict(neighborhood="gaussian", compact_support=True)])
def test_fused_merge_untouched_units(neigh):
    rows = gaussian_blobs(300, 128, seed=13)
    w0 = _codebook(64, 64, 128, 7)
    ref = _compare(64, 64, 128, rows=rows, w0=w0, sigmas=(1.5, 1.5, 1.2, 1.0), **neigh)
    kept = (ref[0][2] == w0).all(axis=1).sum()
    assert 0 < kept < 64 * 64                               # (both kinds of unit are there)


# f: a NaN unit and a unit of 1e30 (|w|^2 overflows): the NaN radius, "left out of the maximum", the scale far from 1
#    (bubble: the two units lie out of every row's reach and stay through the epochs)
def test_fused_merge_nan_and_huge_units():
    rows = gaussian_blobs(600, 128, seed=14)
    w0 = _codebook(64, 64, 128, 8)
    w0[1000] = np.nan
    w0[3000] = 1e30
    w0[77, 5] = 3.0e4                                       # (a finite maximum far from the rest as well)
    _compare(64, 64, 128, rows=rows, w0=w0, sigmas=(1.5, 1.5, 1.2), neighborhood="bubble")


# g: set_weights between two epochs, then a query before the next merge
def test_fused_merge_set_weights_between_epochs():
    rows = gaussian_blobs(N_ROWS, 128, seed=15)
    _compare(64, 64, 128, rows=rows, w0=_codebook(64, 64, 128, 9), sigmas=SIGMAS, reset_after=1)


# h: no plan buffers (SOM_EXACT_SKIP=0) and a merge before any BMU launch: the fused merge without centroids
def test_fused_merge_without_plan_buffers():
    rows = gaussian_blobs(N_ROWS, 128, seed=16)
    _compare(64, 64, 128, rows=rows, w0=_codebook(64, 64, 128, 10), sigmas=SIGMAS, skip=0, forced_first=True)
