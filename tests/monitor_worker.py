"""The training monitor's test double and the gloo worker of tests/test_monitor_cpu.py -- TEST CODE ONLY.

MonitorOracleEngine is OracleEngine + the four monitor calls answered from tests/monitor_ref.py, with a log of the calls it
received and a snapshot per epoch (codebook before, ids, codebook after).  Its accumulator is float64: the sums of two shards then
equal the sum over all rows to float64 rounding, so the merged float32 codebook -- and with it every id and every record -- is the
same however the rows are sharded, which is what the two-rank test compares.  Integer sample weights only (a row of weight m is
accumulated as m copies)."""
import os

import numpy as np

from oracle import som_oracle as O
from tests import monitor_ref as R
from tests.oracle_engine import OracleEngine

F32, F64 = np.float32, np.float64


class MonitorOracleEngine(OracleEngine):
    log = []              # names of the epoch calls, in order, over every instance
    instances = 0

    def __init__(self, *a, missing=None, **kw):
        super().__init__(*a, **kw)
        type(self).instances += 1
        self.acc = np.zeros((self.K, self.D + 1), F64)
        self.device = 0
        self.monitoring = False
        self.weights = self.prev = self.ids = None
        self.m = {}
        self.epochs = []  # (W before, ids, W after) of every merged epoch

    def set_data(self, data):
        super().set_data(data)
        self.weights = self.prev = None

    def set_sample_weights(self, w):
        self.weights = None if w is None else np.asarray(w, F32)
        assert self.weights is None or (self.weights == np.round(self.weights)).all()

    def monitor(self, on=True):
        self.log.append("monitor_on" if on else "monitor_off")
        self.monitoring = bool(on)
        if not on:
            self.prev = None

    def _accumulate(self, sigma, eta, neigh_f64):
        self.acc[:] = 0
        W3 = self.W.reshape(self.x, self.y, self.D)
        self.ids = O.bmu_ids(self.data, self.W, self.kw["distance"]) if self.n_rows else np.zeros(0, np.int64)
        rows, ids = self.data, self.ids
        if self.weights is not None:
            rep = self.weights.astype(np.int64)
            rows, ids = np.repeat(rows, rep, axis=0), np.repeat(ids, rep)
        if len(rows):
            _, num, den = O.update(rows, W3, eta, sigma, wide=bool(neigh_f64), forced_bmu=ids, **self.kw)
            self.acc[:, :self.D] = num.reshape(self.K, self.D)
            self.acc[:, self.D] = den.reshape(self.K)

    def epoch_accumulate(self, sigma, eta, neigh_f64):
        self.log.append("accumulate")
        self._accumulate(sigma, eta, neigh_f64)

    def stream_epoch_accumulate(self, chunks, sigma, eta, neigh_f64):
        self.log.append("stream")
        self.set_data(np.concatenate([np.asarray(c, F32) for c in chunks]))
        self._accumulate(sigma, eta, neigh_f64)
        if self.monitoring:                               # (every chunk measured behind its search; no ids to compare with)
            self.m.update(R.row_metrics(self.data, self.W, self.ids))

    def _merged(self):
        den = self.acc[:, self.D:self.D + 1]
        with np.errstate(all="ignore"):
            return np.where(den != 0, self.acc[:, :self.D] / den, self.W).astype(F32)

    def epoch_measure_rows(self):
        self.log.append("measure_rows")
        assert self.monitoring
        self.m.update(R.row_metrics(self.data, self.W, self.ids, self.weights, self.prev))
        self.prev = self.ids.copy()

    def epoch_measure_shift(self):
        self.log.append("measure_shift")
        assert self.monitoring
        sumsq, mx = R.shift(self.W, self._merged())
        self.m.update(shift_sumsq=sumsq, shift_max=float(mx))

    def epoch_merge(self):
        self.log.append("merge")
        before = self.W.copy()
        self.W = self._merged()
        self.epochs.append((before, None if self.ids is None else self.ids.copy(), self.W.copy()))

    def epoch_metrics(self):
        self.log.append("metrics")
        return dict(self.m)


def stop_at(iteration):
    """A callback that is a pure function of the record: stop once `iteration` has run."""
    return lambda rec: rec.iteration >= iteration


def data_rows():
    return O.gaussian_blobs(300, 5, seed=11)


def worker(rank, world, out_dir, stop):
    """One gloo rank: XPySom.train(monitor=True) on its slice of the 300 rows; saves its history."""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), SOM_OVERLAP="0")
    import pickle

    import torch.distributed as dist
    from xpysom_dask_amd import XPySom, engine
    engine.HipEngine = MonitorOracleEngine               # test double in THIS worker process only
    dist.init_process_group("gloo", init_method="file://%s" % os.path.join(out_dir, "rendezvous"), rank=rank, world_size=world)
    try:
        som = XPySom(8, 7, 5, random_seed=3)
        som.train(data_rows(), 6, monitor=True, callback=None if stop is None else stop_at(stop))
        with open(os.path.join(out_dir, "h%d.pkl" % rank), "wb") as f:
            pickle.dump(([tuple(r) for r in som.history], np.asarray(som._weights)), f)
    finally:
        dist.destroy_process_group()
