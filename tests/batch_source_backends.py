"""Stand-ins for HeatflowHIP in the CPU tests of the sweeps under a source with monitors.  TEST CODE: it lives under
tests/ and is never imported by heatflow_amd.

BatchSourceOracleBackend   tests/oracle_backend.OracleBackend with the volumetric source of tests/source_oracle.py and the monitors of
                           tests/monitor_oracle.py, in single runs and in the batched loop (every column on its own)
RecordingBatchBackend      records the calls and their arguments and answers with arrays of the right shape
"""
import math

import numpy as np

import monitor_oracle as mo
import source_oracle as so
from oracle_backend import OracleBackend


class BatchSourceOracleBackend(OracleBackend):
    F1 = None
    amp = ()
    pos = 0
    thresholds = None

    def set_mesh(self, coords, tris, tags, pattern=None):
        super().set_mesh(coords, tris, tags, pattern)
        self.tab_len = int(np.max(tags)) + 1
        self.thresholds, self.records = None, []
        self.calls = []

    # -- the context's own source and monitors (single runs) -------------------------------------------------------------------
    def set_source(self, tags, fwhm=1.0, z0=0.0, depth=math.inf):
        t = [] if tags is None else list(tags)
        self.F1 = so.source_vector(self.coords, self.tris, self.tags, t, fwhm, z0, depth)[0] if t else None
        self.amp, self.pos = (), 0

    def get_source(self):
        return self.F1.copy()

    def set_source_amplitudes(self, p):
        self.amp, self.pos = tuple(float(v) for v in p), 0

    def set_monitors(self, thresholds):
        if getattr(self, "batch_nv", 0):
            raise RuntimeError("hf_set_monitors: a batch is open (the batched loop records nothing)")
        self.thresholds, self.records = dict(thresholds), []

    def _record(self, u):
        return mo.per_tag(self.coords, self.tris, self.tags, u, self.thresholds, self.tab_len)[0]

    def monitor_now(self):
        return self._record(self.u)

    def monitor_count(self):
        return len(self.records)

    def get_monitors(self, first=0, count=None):
        return np.array(self.records[first:None if count is None else first + count]).reshape(-1, self.tab_len, 7)

    def clear_monitor_records(self):
        self.records = []

    def step(self, g, rtol=1e-10, atol=0.0, max_it=20000):
        p = 0.0
        if self.amp:
            p = self.amp[self.pos]
            self.pos += 1
        b = self.M @ self.u + (self._dt * p * self.F1 if self.F1 is not None else 0.0)
        if self.n_bc:
            b -= self.A_lift @ g
            b[self.bc_dofs] = g
        self.u = self._lu.solve(b)
        if self.thresholds:
            self.records.append(self.monitor_now())
        return 1, 0.0

    # -- the open batch's source and records --------------------------------------------------------------------------------------
    def batch_begin(self, nv, per_column_operator=False):
        if self.F1 is not None:
            raise RuntimeError("hf_batch_begin: a source is set (the batched loop has no load term)")
        super().batch_begin(nv, per_column_operator)
        self._bF1, self._bamp, self._bpos, self._bmon, self._brec = None, None, 0, False, []

    def batch_set_source(self, tags, fwhm=1.0, z0=0.0, depth=math.inf):
        self.calls.append(("batch_set_source", list(tags or []), fwhm, z0, depth))
        if not tags:
            self._bF1 = None
            return
        nv = self.batch_nv
        f = np.broadcast_to(np.asarray(fwhm, dtype=np.float64), (nv,))
        d = np.broadcast_to(np.asarray(depth, dtype=np.float64), (nv,))
        self._bF1 = [so.source_vector(self.coords, self.tris, self.tags, list(tags), float(f[j]), z0, float(d[j]))[0] for j in range(nv)]
        self._bamp, self._bpos = None, 0
        self.batch_source_downloads = 0

    def batch_get_source(self, j):
        self.batch_source_downloads += 1
        return self._bF1[j].copy()

    def batch_set_source_amplitudes(self, p):
        p = np.asarray([] if p is None else p, dtype=np.float64)
        self.calls.append(("batch_set_source_amplitudes", p.copy()))
        self._bamp, self._bpos = (p if p.size else None), 0

    def batch_set_monitors(self, on=True):
        if on and not self.thresholds:
            raise RuntimeError("hf_batch_set_monitors: no monitors set")
        self._bmon, self._brec = bool(on), []

    def batch_monitor_now(self):
        return np.array([self._record(c["u"]) for c in self._bcols])

    def batch_monitor_count(self):
        return len(self._brec)

    def batch_get_monitors(self, first=0, count=None):
        return np.array(self._brec[first:None if count is None else first + count]).reshape(-1, self.batch_nv, self.tab_len, 7)

    def batch_run(self, g_all, rtol=1e-10, atol=0.0, max_it=20000, nodes=None, flux_nodes=None, flux_components=2,
                  flux_rtol=None, flux_max_it=5000):
        nsteps, _, nv = g_all.shape
        if self._bF1 is not None and self._bamp is not None and self._bpos + nsteps > len(self._bamp):
            raise RuntimeError("hf_batch_run: the source has too few amplitudes left")
        ns = 0 if nodes is None else len(nodes)
        samples = np.empty((nsteps, nv, ns))
        for s in range(nsteps):
            for j, col in enumerate(self._bcols):
                b = col["M"] @ col["u"]
                if self._bF1 is not None and self._bamp is not None:
                    b = b + self._dt * self._bamp[self._bpos, j] * self._bF1[j]
                if self.n_bc:
                    g = np.ascontiguousarray(g_all[s, :, j])
                    b -= col["lift"] @ g
                    b[self.bc_dofs] = g
                col["u"] = col["lu"].solve(b)
                if ns:
                    samples[s, j] = col["u"][np.asarray(nodes)]
            if self._bF1 is not None and self._bamp is not None:
                self._bpos += 1
            if self._bmon:
                self._brec.append(self.batch_monitor_now())
        return samples, np.ones((nsteps, nv), dtype=np.int32)

    def batch_end(self):
        super().batch_end()
        self._bF1, self._bamp, self._bmon, self._brec = None, None, False, []


class RecordingBatchBackend:
    """Records the HeatflowHIP calls a session makes; the answers have the shapes of the real ones and hold zeros (ones for the
    source vectors, so that their sum is positive)."""

    def __init__(self, n, n_tab):
        self.calls, self.args = [], []
        self.n, self.tab_len, self.batch_nv = n, n_tab, 0

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def rec(*a, **k):
            self.calls.append(name)
            self.args.append(a)
            if name == "batch_begin":
                self.batch_nv = int(a[0])
            if name == "batch_run":
                g = a[0]
                ns = 0 if len(a) < 5 or a[4] is None else len(a[4])
                return np.zeros((g.shape[0], g.shape[2], ns)), np.ones((g.shape[0], g.shape[2]), dtype=np.int32)
            if name == "batch_get_source":
                return np.ones(self.n)
            if name == "batch_get_monitors":
                return np.zeros((self._steps(), self.batch_nv, self.tab_len, 7))
            return None
        return rec

    def _steps(self):
        for name, a in zip(reversed(self.calls), reversed(self.args)):
            if name == "batch_run":
                return a[0].shape[0]
        return 0
