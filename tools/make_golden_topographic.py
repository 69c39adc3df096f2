#!/usr/bin/env python3
"""Generator of tests/golden/g21_topographic_64x64x32.npz -- runs only where the reference implementation is importable
(REFERENCE_PATH names its checkout; imported at generation time, nothing of it is copied or shipped, as in
oracle/make_golden.py).  The fixture is data: a codebook the reference trained for a few epochs, the seed of the probe
rows, the reference's topographic_error on them, and every probe row's two smallest distances.

    REFERENCE_PATH=<checkout of the reference> python tools/make_golden_topographic.py [X Y D]

The reference takes the best-2 pair from an unstable argsort of the float32 distance matrix (xpysom.py:727-734), so the
fixture pins VALUES (the two smallest distances); `distinct` marks the rows whose two smallest float32 distances differ
from each other and from the third -- only there the pair of ids is pinned too.
"""
import contextlib
import io
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True
with contextlib.redirect_stdout(io.StringIO()):
    sys.path.insert(0, os.environ["REFERENCE_PATH"])
    from xpysom_dask import XPySom as RefSom                                   # noqa: E402

from oracle.som_oracle import gaussian_blobs                                   # noqa: E402
from tests.top2_ref import unsettled_share                                     # noqa: E402

F32 = np.float32


def main():
    X, Y, D = (int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (64, 64, 32)
    # (gaussian_blobs draws its centres from the seed: the probe takes the TRAINING seed with another row count -- the same
    #  mixture, other rows; rows of another mixture sit far from every unit, where no SOM quality figure means much)
    train_seed, probe_seed, n_train, n_probe, epochs = 210, 210, 8192, 4096, 4
    data = gaussian_blobs(n_train, D, seed=train_seed)
    with contextlib.redirect_stdout(io.StringIO()):
        som = RefSom(X, Y, D, sigma=X / 4.0, learning_rate=0.5, random_seed=21, n_parallel=n_train, xp=np)
        som.train(data, epochs)
    probe = gaussian_blobs(n_probe, D, seed=probe_seed)
    assert not np.array_equal(probe, data[:n_probe])
    w = som._weights.astype(F32)
    som._weights = w
    dist = np.asarray(som._distance_from_weights(probe.astype(F32), w), F32)
    order = np.argsort(dist, axis=1, kind="stable")[:, :3]
    r = np.arange(n_probe)
    d3 = dist[r[:, None], order]
    distinct = (d3[:, 0] < d3[:, 1]) & (d3[:, 1] < d3[:, 2])
    te = np.float64(som.topographic_error(probe))
    # the share of these rows the exact mode's tie test would hand to the float32 top-2 kernel (CPU estimate, tests/top2_ref.py):
    # the GPU test asserts the fast path on this fixture, so the inputs are checked for it HERE, before they are fixed
    share = unsettled_share(probe, w.reshape(-1, D))
    assert share <= 0.01, share
    path = os.path.join(REPO, "tests", "golden", "g21_topographic_%dx%dx%d.npz" % (X, Y, D))
    np.savez_compressed(path, w=w, probe_seed=np.array(probe_seed), n_probe=np.array(n_probe), te=te, d12=d3[:, :2].astype(F32),
                        ids12=order[:, :2].astype(np.int32), distinct=distinct, unsettled_share_cpu=np.float64(share))
    print("%s %.1f KB; te = %r; %d of %d rows distinct; unsettled share (CPU estimate) %r" % (
        path, os.path.getsize(path) / 1024, float(te), int(distinct.sum()), n_probe, share))


if __name__ == "__main__":
    main()
