#!/usr/bin/env python3
"""BASELINE configs[0]: the Iris walk-through of the reference (examples/Iris.ipynb) on the MI355X engine.

    python examples/iris.py            # needs libsomhip.so and a GPU

6x6 map, 4 features, 150 samples z-scored, 100 epochs -- the same calls a user of xpysom_dask.XPySom makes; only the
import changes.  The data come from the fixture the parity tests use (tests/golden/g6_iris.npz holds the reference's
iris.csv columns and, for comparison, the reference's own quantization errors for this run).
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from xpysom_dask_amd import XPySom  # noqa: E402   (reference: from xpysom_dask import XPySom)

g = np.load(os.path.join(REPO, "tests", "golden", "g6_iris.npz"))
raw = g["iris_raw"]
data = (raw - raw.mean(axis=0)) / raw.std(axis=0)

for decay in ("linear", "exponential"):
    som = XPySom(6, 6, 4, random_seed=10, decay_function=decay)
    print("%-12s quantization error before training: %.5f" % (decay, som.quantization_error(data)))
    som.train(data, 100, monitor=True)      # the learning curve comes with the training: one EpochRecord per epoch in som.history
    for r in som.history[::20] + som.history[-1:]:
        print("%-12s epoch %3d  sigma %.3f  QE %.5f  BMU changes %s  codebook shift %.5f"
              % (decay, r.iteration, r.sigma, r.quantization_error, r.bmu_changed, r.codebook_shift))
    qe = som.quantization_error(data)
    print("%-12s after 100 epochs: %.5f   (reference: %.5f)   topographic error %.4f"
          % (decay, qe, float(g[decay + "_default_qe"]), som.topographic_error(data)))
    wins = som.winner(data)
    print("%-12s first five winners: %s" % (decay, wins[:5]))
    hits = som.activation_response(data)
    print("%-12s busiest unit holds %d of 150 samples; %d of 36 units win at least one" % (decay, hits.max(), (hits > 0).sum()))
    # the label map: iris.csv lists 50 setosa, 50 versicolor, 50 virginica in that order (class codes 0, 1, 2)
    species = np.repeat(np.arange(3), 50)
    counts = som.label_counts(data, species)                # (6, 6, 3): how many samples of each species every unit wins
    print("%-12s label map (majority species per unit, . = no sample):" % decay)
    for row in np.where(counts.sum(axis=2) > 0, counts.argmax(axis=2), -1):
        print("%-12s   %s" % ("", " ".join("." if c < 0 else str(c) for c in row)))
    print("%-12s classify on the training samples: accuracy %.3f" % (decay, (som.classify(data, counts) == species).mean()))
    petal = som.unit_means(data, raw[:, 2])                 # a component plane: the mean raw petal length per unit
    print("%-12s mean petal length per unit: %.2f ... %.2f cm" % (decay, np.nanmin(petal.mean), np.nanmax(petal.mean)))
