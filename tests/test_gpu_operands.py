"""Stale codebook operands on the device: an engine that has trained, merged, switched between its kernels and had its codebook
replaced must answer every query exactly as a FRESH engine of the same configuration does from the same codebook -- a fresh engine
has every operand stale by construction and rebuilds all it reads (csrc/codebook_operands.hpp keeps the books; the CPU suite
checks them against a model, tests/test_operands_cpu.py; here the kernels read what the books say is current).

Per case a seeded script of 24 steps drawn from set_weights, epoch_accumulate + epoch_merge, bmu, bmu(quantization=True),
bmu_top2, quantization_error and distance_matrix; behind every query step the fresh engine gets get_weights() and answers the same
query: ids and distance matrices bit for bit, the quantization error as a float64 value.  Cases: the smallest shapes that reach
each branch (float32 stage / tile image, the half-fused merge and cosine's |w|^2, patch order with and without the 4 x 4
sub-blocks and the permute's scalar path, the deferred image and the fused merge with centroids under SOM_EXACT_SKIP=2, the
wide path's five feature chunks, a replayed graph's bookkeeping)."""
import contextlib
import os

import numpy as np
import pytest

from xpysom_dask_amd.synthetic import gaussian_blobs

pytestmark = pytest.mark.gpu

N_QUERY = 256
SIGMAS = (4.0, 3.0, 2.5, 2.0, 1.5, 1.2, 1.0, 0.8)
QUERIES = ("bmu", "bmu_q", "top2", "qe", "dm")

#        id                      x   y   d    precision distance     env                      resident rows, graph script
CASES = [
    ("f32-8x8x8",                8,  8,  8,   "f32",   "euclidean", {},                       1024, False),
    ("f32-8x8x130",              8,  8,  130, "f32",   "euclidean", {},                       1024, False),
    ("bf16-8x8x8",               8,  8,  8,   "bf16",  "euclidean", {},                       1024, False),
    ("bf16-cosine-8x8x8",        8,  8,  8,   "bf16",  "cosine",    {},                       1024, False),
    ("exact-16x16x8-skip2",      16, 16, 8,   "exact", "euclidean", {"SOM_EXACT_SKIP": "2"},  1024, False),
    ("exact-12x11x5-skip2",      12, 11, 5,   "exact", "euclidean", {"SOM_EXACT_SKIP": "2"},  1024, False),
    ("exact-16x16x8-skip0",      16, 16, 8,   "exact", "euclidean", {"SOM_EXACT_SKIP": "0"},  1024, False),
    ("exact-64x64x260",          64, 64, 260, "exact", "euclidean", {},                       512,  False),
    ("exact-cosine-64x64x260",   64, 64, 260, "exact", "cosine",    {},                       512,  False),
    ("f32-12x9x7-graph",         12, 9,  7,   "f32",   "euclidean", {"SOM_GRAPH": "1"},       1024, True),
    ("bf16-cosine-12x9x7-graph", 12, 9,  7,   "bf16",  "cosine",    {"SOM_GRAPH": "1"},       1024, True),
]


@contextlib.contextmanager
def _env(kv):
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


def _script(seed, graph):
    """24 steps.  graph: one set_weights, then six epochs with nothing but queries between them (a replay's bookkeeping is what the
    next reader finds); else every kind of step anywhere, the codebook replaced now and then."""
    rng = np.random.default_rng(seed)
    if graph:
        steps = ["set_weights"]
        for _ in range(6):
            steps += ["epoch"] + list(rng.choice(QUERIES, size=3))
        return steps[:24]
    kinds = ("set_weights", "epoch", "epoch") + QUERIES
    return ["set_weights"] + list(rng.choice(kinds, size=23))


def _query(eng, kind, rows):
    if kind == "bmu":
        return (eng.bmu(rows),)
    if kind == "bmu_q":
        return (eng.bmu(rows, quantization=True),)
    if kind == "top2":
        return eng.bmu_top2(rows)
    if kind == "qe":
        return (np.float64(eng.quantization_error(rows)),)
    return (eng.distance_matrix(rows, quantization=True), eng.distance_matrix(rows))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_queries_match_a_fresh_engine(case):
    from xpysom_dask_amd.engine import HipEngine
    name, x, y, d, precision, distance, env, n_rows, graph = case
    seed = CASES.index(case)

    def engine():
        with _env(env):                                   # (the library reads the switches in som_create)
            return HipEngine(x, y, d, precision=precision, distance=distance)

    data = np.abs(gaussian_blobs(n_rows, d, seed=100 + seed)) + 0.25      # (away from the origin: cosine's unit-length rows exist)
    rows = np.ascontiguousarray(data[:N_QUERY] * 1.01 + 0.01, dtype=np.float32)
    rng = np.random.default_rng(200 + seed)
    eng = engine()
    try:
        eng.set_data(data)
        epochs = 0
        for step, kind in enumerate(_script(seed, graph)):
            if kind == "set_weights":
                eng.set_weights(np.abs(rng.normal(0.0, 1.0, size=(x * y, d))).astype(np.float32) + 0.05)
            elif kind == "epoch":
                eng.epoch_accumulate(SIGMAS[epochs % len(SIGMAS)], 0.5, 1)
                eng.epoch_merge()
                epochs += 1
            else:
                got = _query(eng, kind, rows)
                fresh = engine()
                try:
                    fresh.set_weights(eng.get_weights())
                    want = _query(fresh, kind, rows)
                finally:
                    fresh.close()
                for g, w in zip(got, want):
                    assert np.array_equal(g, w), "%s: step %d (%s) differs from a fresh engine's answer" % (name, step, kind)
    finally:
        eng.close()
