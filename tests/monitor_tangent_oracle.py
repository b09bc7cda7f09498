"""Float64 restatement of the monitor derivatives (hf_set_monitor_tangents).  TEST CODE.

Per triangle the derivative terms are formed with the operations of monitor_term_tan in their pinned order (numpy evaluates one
IEEE operation per ufunc call, nothing is contracted); per tag they are summed with math.fsum, so only the order of summation
differs from the device.  dT_max / dT_min are exact: the tangent at the node of the primal record.  ``scale`` is, per tag and
field, the sum over the triangles of the term with every product taken in absolute value (the terms cancel internally, so |term|
alone is not a sound scale); the bound is the project's, (ne_t + 16) 2^-52 scale.
"""
import math

import numpy as np

import monitor_oracle as mo

FIELDS = ("dT_max", "dT_min", "dI0", "dI1", "dH")
EPS = mo.EPS

# Central differences of two primal monitor runs against the derivative records (tests/test_monitor_tangents_cpu.py on the scipy
# stand-in, tests/test_gpu_monitor_tangents.py on the GPU).  The run: 10 steps of 375 ns - the first ends past the first sample of
# the heating curve (357 ns), so every step is heated, and the run ends while the pulse (peak at 1.93 us) still holds every
# region's peak on one node.  The coupler monitored is the o-side one: the p-side coupler's peak sits on the heated line, a
# Dirichlet node, where every derivative is an exact zero.  FD_REL_STEP is the relative step found in float64 by the rule of DESIGN.md
# 3.15 (start at 1e-3, halve until the difference is within a quarter of 1e-4 of the largest derivative over the steps), FD_FLOAT64
# the largest difference any compared field (T_mean, energy, T_max of both regions, both small meshes) reaches at it in float64,
# FD_TOL the project's tolerance for tangents against central differences (test_gpu_capacity_tangent.py).
FD_NSTEPS, FD_T_FINAL = 10, 3.75e-6
FD_MONITORS = {"sample": {"material": "p_sample", "above": 300.4}, "coupler": {"material": "o_coupler"}}
FD_REL_STEP = {"p_sample": 1e-3, "p_sample.rho_c": 1e-3, "p_sample.thickness": 1e-3}
FD_FLOAT64 = {"p_sample": 2.5e-7, "p_sample.rho_c": 3.1e-7, "p_sample.thickness": 2.1e-6}
FD_TOL = 1e-4


def triangle_tangent_terms(coords, tris, u, theta, t, v=None):
    """(dI0_e, dI1_e, dH_e) of every triangle for one column with nodal tangent ``t`` and (shape columns) nodal z-velocity
    ``v``, and the three scales (every product in absolute value); ``theta`` per triangle (+inf: nothing is above)."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64), (len(tris),))
    z = coords[tris, 0]
    r = coords[tris, 1]
    uu = u[tris]
    tt = t[tris]
    z0, z1, z2 = z[:, 0], z[:, 1], z[:, 2]
    r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
    u0, u1, u2 = uu[:, 0], uu[:, 1], uu[:, 2]
    t0, t1, t2 = tt[:, 0], tt[:, 1], tt[:, 2]
    d = (z1 - z0) * (r2 - r0) - (z2 - z0) * (r1 - r0)
    A = 0.5 * np.abs(d)
    rs = (r0 + r1) + r2
    I0 = (A * rs) / 3.0
    I1 = (A / 12.0) * (((rs + r0) * u0 + (rs + r1) * u1) + (rs + r2) * u2)
    I1_abs = (A / 12.0) * ((np.abs(rs + r0) * np.abs(u0) + np.abs(rs + r1) * np.abs(u1)) + np.abs(rs + r2) * np.abs(u2))
    J1 = (A / 12.0) * (((rs + r0) * t0 + (rs + r1) * t1) + (rs + r2) * t2)
    J1_abs = (A / 12.0) * ((np.abs(rs + r0) * np.abs(t0) + np.abs(rs + r1) * np.abs(t1)) + np.abs(rs + r2) * np.abs(t2))
    above = uu > theta[:, None]
    cnt = above.sum(axis=1)
    odd = cnt == 1
    a = np.where(above[:, 0] == odd, 0, np.where(above[:, 1] == odd, 1, 2))
    rows = np.arange(len(tris))
    b, c = (a + 1) % 3, (a + 2) % 3
    ua, ub, uc = uu[rows, a], uu[rows, b], uu[rows, c]
    ra, rb, rc = r[rows, a], r[rows, b], r[rows, c]
    ta, tb, tc = tt[rows, a], tt[rows, b], tt[rows, c]
    cut_case = (cnt == 1) | (cnt == 2)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sb = (ua - theta) / (ua - ub)
        sc = (ua - theta) / (ua - uc)
        G = (ra + (ra + sb * (rb - ra))) + (ra + sc * (rc - ra))
        cut = (((A * sb) * sc) * G) / 3.0
        pb = ((1.0 - sb) * ta + sb * tb) / (ua - ub)
        pc = ((1.0 - sc) * ta + sc * tc) / (ua - uc)
        dcut = (A * ((pb * sc + sb * pc) * G + (sb * sc) * (pb * (rb - ra) + pc * (rc - ra)))) / 3.0
        pb_abs = (np.abs(1.0 - sb) * np.abs(ta) + np.abs(sb) * np.abs(tb)) / np.abs(ua - ub)
        pc_abs = (np.abs(1.0 - sc) * np.abs(ta) + np.abs(sc) * np.abs(tc)) / np.abs(ua - uc)
        dcut_abs = (A * ((pb_abs * np.abs(sc) + np.abs(sb) * pc_abs) * np.abs(G)
                         + np.abs(sb * sc) * (pb_abs * np.abs(rb - ra) + pc_abs * np.abs(rc - ra)))) / 3.0
    H = np.where(cnt == 3, I0, np.where(cut_case, np.where(odd, cut, I0 - cut), 0.0))
    H_abs = np.where(cnt == 3, I0, np.where(cut_case, np.where(odd, np.abs(cut), I0 + np.abs(cut)), 0.0))
    dH = np.where(cut_case, np.where(odd, dcut, -dcut), 0.0)
    dH_abs = np.where(cut_case, dcut_abs, 0.0)
    dI0, dI1 = np.zeros(len(tris)), J1
    dI0_abs, dI1_abs = np.zeros(len(tris)), J1_abs
    if v is not None:
        vv = np.asarray(v, dtype=np.float64)[tris]
        v0, v1, v2 = vv[:, 0], vv[:, 1], vv[:, 2]
        dd = (v1 - v0) * (r2 - r0) - (v2 - v0) * (r1 - r0)
        q = dd / d
        q_abs = (np.abs(v1 - v0) * np.abs(r2 - r0) + np.abs(v2 - v0) * np.abs(r1 - r0)) / np.abs(d)
        dI0 = q * I0
        dI1 = J1 + q * I1
        dH = dH + q * H
        dI0_abs = q_abs * I0
        dI1_abs = J1_abs + q_abs * I1_abs
        dH_abs = dH_abs + q_abs * H_abs
    return (dI0, dI1, dH), (dI0_abs, dI1_abs, dH_abs), cnt


def per_tag_tangent(coords, tris, tags, u, thresholds, s, shape=None, tab_len=None, primal=None):
    """The derivative row [tab_len, nv, 5] of HeatflowHIP.monitor_tangent_eval for the tangent fields ``s`` [n, nv] and ``shape``
    = {column: nodal z-velocity}; per tag ``scale`` [tab_len, nv, 3] (dI0, dI1, dH) and ``ne`` [tab_len].  ``primal`` is the
    primal record whose node ids place dT_max / dT_min (default: the restatement's own)."""
    tags = np.asarray(tags, dtype=np.int64)
    tris = np.asarray(tris, dtype=np.int64)
    s = np.asarray(s, dtype=np.float64)
    shape = dict(shape or {})
    tab_len = int(tags.max()) + 1 if tab_len is None else int(tab_len)
    if primal is None:
        primal = mo.per_tag(coords, tris, tags, u, thresholds, tab_len)[0]
    th_tag = np.full(tab_len, np.nan)
    for t, th in thresholds.items():
        th_tag[int(t)] = math.inf if th is None else float(th)
    theta = np.where(~np.isnan(th_tag[tags]), th_tag[tags], math.inf)
    nv = s.shape[1]
    row = np.zeros((tab_len, nv, 5))
    scale = np.zeros((tab_len, nv, 3))
    ne = np.zeros(tab_len, dtype=np.int64)
    sels = {int(t): tags == int(t) for t in thresholds}
    for j in range(nv):
        terms, scales, _ = triangle_tangent_terms(coords, tris, u, theta, s[:, j], shape.get(j))
        for t, sel in sels.items():
            row[t, j, 0] = s[int(primal[t, 1]), j]
            row[t, j, 1] = s[int(primal[t, 3]), j]
            for f in range(3):
                row[t, j, 2 + f] = math.fsum(terms[f][sel])
                scale[t, j, f] = math.fsum(scales[f][sel])
            ne[t] = int(sel.sum())
    return row, scale, ne


def sum_bound(ne, scale):
    """(ne_t + 16) 2^-52 scale, for scale [tab_len, nv, 3]."""
    return (np.asarray(ne, dtype=np.float64)[:, None, None] + 16.0) * EPS * np.asarray(scale)


def check_row(row, ref, scale, ne, thresholds, label=""):
    """A device derivative row against the restatement: sums within the bound, dT_max / dT_min exact, unmonitored rows exact
    zeros.  Returns the worst error / bound of (dI0, dI1, dH)."""
    bound = sum_bound(ne, scale)
    on = sorted(int(t) for t in thresholds)
    off = [t for t in range(row.shape[0]) if t not in on]
    err = np.abs(row[:, :, 2:] - ref[:, :, 2:])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))[on]
    worst = ratio.reshape(-1, 3).max(axis=0)
    print(f"{label}: worst error / bound  dI0 {worst[0]:.3f}  dI1 {worst[1]:.3f}  dH {worst[2]:.3f}")
    assert np.all(err[on] <= bound[on]), (label, worst)
    assert np.array_equal(row[on, :, :2], ref[on, :, :2]), label
    assert np.all(row[off] == 0.0), label
    return worst


# ---- the scipy stand-in, extended by the monitors and the four new calls ------------------------------------------------------------------
from capacity_tangent_oracle import CapacityTangentOracleBackend  # noqa: E402


class MonitorTangentOracleBackend(CapacityTangentOracleBackend):
    """CapacityTangentOracleBackend (sparse LU; conductivity, directional, shape and capacity columns) with the monitors of the
    restatement after every step of run_tangent and the four calls of the derivative records: set_monitor_tangents,
    monitor_tangent_count, get_monitor_tangents, monitor_tangent_eval."""

    def set_mesh(self, coords, tris, tags, pattern=None):
        super().set_mesh(coords, tris, tags, pattern)
        self.tab_len = int(np.max(tags)) + 1
        self.thresholds, self.records = None, []
        self._mt_on, self._mt_records, self._mt_index = False, [], []
        self._in_tangent_run = False

    def step(self, g, rtol=1e-10, atol=0.0, max_it=20000):
        out = super().step(g, rtol, atol, max_it)
        if self.thresholds and not self._in_tangent_run:      # (run_tangent below records its steps itself)
            self.records.append(self.monitor_now())
        return out

    # the primal monitors
    def set_monitors(self, thresholds):
        self.thresholds, self.records = dict(thresholds or {}) or None, []
        self._mt_on, self._mt_records, self._mt_index = False, [], []

    def monitor_now(self):
        return mo.per_tag(self.coords, self.tris, self.tags, self.u, self.thresholds, self.tab_len)[0]

    def monitor_count(self):
        return len(self.records)

    def get_monitors(self, first=0, count=None):
        return np.array(self.records[first:None if count is None else first + count]).reshape(-1, self.tab_len, 7)

    def clear_monitor_records(self):
        self.records, self._mt_records, self._mt_index = [], [], []

    # the derivative records
    def set_monitor_tangents(self, on):
        if on and not self.thresholds:
            raise RuntimeError("hf_set_monitor_tangents: no monitors set (hf_set_monitors first)")
        self._mt_on = bool(on)

    def monitor_tangent_count(self):
        return len(self._mt_records), (self._mt_records[0].shape[1] if self._mt_records else 0)

    def get_monitor_tangents(self, first=0, count=None):
        count = len(self._mt_records) - first if count is None else count
        nv = self._mt_records[0].shape[1] if self._mt_records else 0
        out = np.array(self._mt_records[first:first + count]).reshape(count, self.tab_len, nv, 5)
        return out, np.asarray(self._mt_index[first:first + count], dtype=np.int32)

    def monitor_tangent_eval(self, s, shape=None):
        return per_tag_tangent(self.coords, self.tris, self.tags, self.u, self.thresholds, s, shape, self.tab_len)[0]

    def run_tangent(self, g_all, h_all=None, rtol=1e-10, atol=0.0, max_it=20000, nodes=None):
        if not self.thresholds:
            return super().run_tangent(g_all, h_all, rtol, atol, max_it, nodes)
        if self._mt_records and self._mt_records[0].shape[1] != self.tangent_nv:
            self._mt_records, self._mt_index = [], []
        parts = []
        for k in range(len(g_all)):        # step by step: the record of every step's state, then the derivatives along its tangents
            self._in_tangent_run = True
            try:
                parts.append(super().run_tangent(g_all[k:k + 1], None if h_all is None else h_all[k:k + 1], rtol, atol, max_it, nodes))
            finally:
                self._in_tangent_run = False
            self.records.append(self.monitor_now())
            if self._mt_on:
                self._mt_records.append(self.monitor_tangent_eval(self.S, dict(self._shape)))
                self._mt_index.append(len(self.records) - 1)
        return tuple(np.concatenate([p[q] for p in parts], axis=0) for q in range(4))
