"""Float64 restatement of tangent runs under the volumetric source (hf_source_derivatives, hf_tangent_set_source)
for the CPU and GPU tests, built on tests/source_oracle.py.  TEST CODE: never imported by heatflow_amd.

    s     = exp(-(c_r r^2 + |z - z0| / depth)),  c_r = 4 ln2 / fwhm^2
    s_f   = ds/dfwhm  = s (2 c_r r^2 / fwhm)
    s_d   = ds/ddepth = s |z - z0| / depth^2            (0 for a uniform layer)
    G_f   = M1 s_f,  G_d = M1 s_d                       (M1: the unit-capacity mass of the absorbing elements, as F1 = M1 s)
    p_k   = P pulse_k / (2 pi sum F1)
    load of a source column at step k: c0 F1 + c1 G_f + c2 G_d = d(p_k F1)/dtheta, added to F_j of the tangent stage
    A s_j^{n+1} = M(...) + dt' F_j, with the scheme's own M(...) and dt' and no other factor.

The nodal values are formed in the device's order of operations, so the restated vectors differ from the device's by the exp
routine, three multiplications per node and the rounding of the row sums.
"""
import math

import numpy as np

import source_oracle as so
from capacity_tangent_oracle import CapacityTangentOracleBackend
from monitor_tangent_oracle import MonitorTangentOracleBackend

SOURCE_PARAMS = ("source.power", "source.fwhm", "source.depth", "source.pulse.t0", "source.pulse.fwhm")

# The relative step of the central differences in the source's parameters, found by tests/test_source_tangent_cpu.py with the rule
# of DESIGN.md 3.15 ("start at 1e-3, halve until the float64 difference is within a quarter of 1e-4 of max|s|"), and used by the
# GPU test too
FD_REL_STEP = {"source.power": 1e-3, "source.fwhm": 1e-3, "source.depth": 1e-3, "source.pulse.t0": 1e-3, "source.pulse.fwhm": 1e-3}


def shape_derivatives(coords, fwhm, z0, depth):
    """(s_f, s_d) at every node, in the kernel's order of operations."""
    zr = np.asarray(coords, dtype=np.float64)
    c_r = 4.0 * math.log(2.0) / (fwhm * fwhm)
    inv_depth = 0.0 if math.isinf(depth) else 1.0 / depth
    s = so.source_shape(zr, fwhm, z0, depth)
    s_f = s * (((2.0 * c_r) * (zr[:, 1] * zr[:, 1])) / fwhm)
    s_d = s * ((np.abs(zr[:, 0] - z0) * inv_depth) * inv_depth)
    return s_f, s_d


def derivative_vectors(coords, tris, tags, absorbing, fwhm, z0, depth=math.inf):
    """(G_f, scale_f, G_d, scale_d): G = M1 g and scale_i = sum_j |M1_ij| |g_j|, the magnitude a rounding bound on G_i is stated
    against."""
    M1 = so.absorbing_mass(coords, tris, tags, absorbing)
    s_f, s_d = shape_derivatives(coords, fwhm, z0, depth)
    return M1 @ s_f, abs(M1) @ np.abs(s_f), M1 @ s_d, abs(M1) @ np.abs(s_d)


def coefficient_table(power, t0, w, times, F1, G_f, G_d, names=SOURCE_PARAMS):
    """{name: (n_steps, 3)} of (c0, c1, c2) for a Gaussian pulse (t0, w) of peak ``power``, restated from the formulas above."""
    t = np.asarray(times, dtype=np.float64)
    S, S_f, S_d = math.fsum(F1), math.fsum(G_f), math.fsum(G_d)
    pulse = so.gaussian_pulse(t, t0, w)
    p = power * pulse / (2.0 * math.pi * S)
    zero = np.zeros(len(t))
    ln2_8 = 8.0 * math.log(2.0)
    table = {
        "source.power": (p / power, zero, zero),
        "source.fwhm": (-p * S_f / S, p, zero),
        "source.depth": (-p * S_d / S, zero, p),
        "source.pulse.t0": (p * ln2_8 * (t - t0) / w ** 2, zero, zero),
        "source.pulse.fwhm": (p * ln2_8 * (t - t0) ** 2 / w ** 3, zero, zero),
    }
    return {nm: np.stack(table[nm], axis=1) for nm in names}


class SourceTangentMixin:
    """The source and its tangent calls on top of a tangent stand-in: set_source, get_source, set_source_amplitudes,
    source_derivatives, get_source_derivative, tangent_set_source; the primal step carries dt' p_k F1, the loads of the source
    columns c0 F1 + c1 G_f + c2 G_d.  The refusals of the library that the Python layers rely on are restated as RuntimeError.
    ``source_calls`` records the names of the source calls made, in order."""

    def set_mesh(self, *a, **kw):
        super().set_mesh(*a, **kw)
        self.F1, self._src, self._diff = None, None, False
        self._amp, self._apos = (), 0
        self._scoef, self._spos, self._scur = None, 0, None
        self._src_tan = False
        self.source_calls = getattr(self, "source_calls", [])

    def set_source(self, tags, fwhm=1.0, z0=0.0, depth=math.inf):
        self.source_calls.append("set_source")
        self._diff, self._scoef, self._scur = False, None, None
        self._amp, self._apos = (), 0
        if not tags:
            self.F1 = self._src = None
            return
        self._src = (list(tags), float(fwhm), float(z0), float(depth))
        self.F1 = so.source_vector(self.coords, self.tris, self.tags, *self._src)[0]

    def get_source(self):
        self.source_calls.append("get_source")
        return self.F1.copy()

    def set_source_amplitudes(self, p):
        self.source_calls.append("set_source_amplitudes")
        self._amp, self._apos = tuple(float(v) for v in p), 0

    def source_derivatives(self, on=True):
        self.source_calls.append("source_derivatives")
        if self.F1 is None:
            raise RuntimeError("hf_source_derivatives: no source set (hf_set_source first)")
        self._scoef, self._scur = None, None
        self._diff = bool(on)
        if on:
            self.Gf, _, self.Gd, _ = derivative_vectors(self.coords, self.tris, self.tags, *self._src)

    def get_source_derivative(self, which):
        self.source_calls.append("get_source_derivative")
        if not self._diff:
            raise RuntimeError("hf_get_source_derivative: the source is not differentiable (hf_source_derivatives first)")
        return (self.Gf if {"fwhm": 0, "depth": 1}.get(which, which) == 0 else self.Gd).copy()

    def _refuse_plain_source(self, call):
        if self.F1 is not None and not self._diff:
            raise RuntimeError(f"{call}: a source is set (hf_set_source; tangents of sourced runs are not supported)")

    def tangent_setup(self, n_par, tag_col):
        self._refuse_plain_source("hf_tangent_setup")
        super().tangent_setup(n_par, tag_col)
        self._scoef, self._scur = None, None

    def tangent_setup_dir(self, n_par, k=None, r=None, z=None):
        self._refuse_plain_source("hf_tangent_setup_dir")
        super().tangent_setup_dir(n_par, k, r, z)
        self._scoef, self._scur = None, None

    def tangent_set_source(self, coef):
        self.source_calls.append("tangent_set_source")
        if not self.tangent_nv or not self._diff:
            raise RuntimeError("hf_tangent_set_source: no set-up, or the source is not differentiable")
        self._scoef, self._spos, self._scur = None, 0, None
        if coef is not None and len(coef):
            c = np.array(coef, dtype=np.float64)
            if c.ndim != 3 or c.shape[1:] != (self.tangent_nv, 3) or not np.all(np.isfinite(c)):
                raise ValueError("hf_tangent_set_source: (n_steps, nv, 3) finite coefficients expected")
            self._scoef = c

    def _reset_tangents(self):
        super()._reset_tangents()
        self._scur = None

    def step(self, g, rtol=1e-10, atol=0.0, max_it=20000):
        if self.F1 is None:
            return super().step(g, rtol, atol, max_it)
        p = 0.0
        if self._amp:
            if self._apos >= len(self._amp):
                raise RuntimeError("the source has 0 amplitudes left (hf_set_source_amplitudes)")
            p = self._amp[self._apos]
            self._apos += 1
        if self._src_tan and self._scoef is not None:
            self._scur = self._spos
            self._spos += 1
        keep = self._load
        self._load = p * self.F1 if keep is None else keep + p * self.F1
        try:
            return super().step(g, rtol, atol, max_it)
        finally:
            self._load = keep

    def source_terms(self, j):
        """(c0 F1 + c1 G_f + c2 G_d, the sum of the absolute terms) of column j at the coefficients of the last step taken (zeros
        where none was)."""
        if self._scoef is None or self._scur is None:
            return np.zeros(self.n), np.zeros(self.n)
        c0, c1, c2 = self._scoef[self._scur, j]
        return ((c0 * self.F1 + c1 * self.Gf) + c2 * self.Gd,
                (abs(c0) * np.abs(self.F1) + abs(c1) * np.abs(self.Gf)) + abs(c2) * np.abs(self.Gd))

    def _loads(self, mats, w):
        F, T = super()._loads(mats, w)
        if self._scoef is not None and self._scur is not None:
            for j in range(self.tangent_nv):
                f, t = self.source_terms(j)
                F[:, j] = F[:, j] + f
                T[:, j] += t
        return F, T

    def run_tangent(self, g_all, h_all=None, rtol=1e-10, atol=0.0, max_it=20000, nodes=None):
        self._refuse_plain_source("hf_run_tangent")
        if self.F1 is not None and any(np.any(v != 0.0) for v in self._shape.values()):
            raise RuntimeError("hf_run_tangent: a source is set and a column has a shape part")
        if self._scoef is not None and self._spos + len(g_all) > len(self._scoef):
            raise RuntimeError("hf_run_tangent: the source columns have too few rows left (hf_tangent_set_source)")
        # the loop that goes through _loads runs only with a shape column: an all-zero velocity on column 0 adds exact zeros
        trick = self._scoef is not None and not self._shape
        if trick:
            self._shape = {0: np.zeros(self.n)}
        self._src_tan = True
        try:
            return super().run_tangent(g_all, h_all, rtol, atol, max_it, nodes)
        finally:
            self._src_tan = False
            if trick:
                self._shape = {}


class SourceTangentOracleBackend(SourceTangentMixin, CapacityTangentOracleBackend):
    """Sparse-LU stand-in with conductivity, directional, capacity and source columns."""


class SourceMonitorOracleBackend(SourceTangentMixin, MonitorTangentOracleBackend):
    """The same with the region monitors and their derivative records."""


# ---- shared set-up of the CPU and GPU tests -------------------------------------------------------------------------------------------------
NSTEPS = 20
FWHM = 1.4e-5      # as tests/test_gpu_source.py: 4 ln2 r^2 / fwhm^2 <= 100 on both small meshes


def beam(case, names=("p_coupler",), depth=2.0e-8, power=0.2, fwhm=FWHM, t0_steps=10.0, w_steps=8.0):
    """The parameters of a pulsed source on ``case`` = (cfg, stack, mesh): the materials, the five differentiable numbers (the
    pulse peaks at step ``t0_steps`` and is ``w_steps`` steps wide) and z0, the outer face of the first material."""
    cfg, stack, _ = case
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    return {"names": tuple(names), "power": float(power), "fwhm": float(fwhm), "depth": float(depth), "t0": t0_steps * dt,
            "w": w_steps * dt, "z0": float(stack.by_name(names[0]).boundaries[0])}


def problem(case, P, keep_line, **kw):
    """A HeatProblem on ``case`` with the source of ``P``: the three outer edges at ic_temp, plus the heated line when
    ``keep_line``."""
    from helpers import material_tables, reference_bcs
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = case
    bcs, ic, heat = reference_bcs(cfg, stack, mesh)
    tk, trc = material_tables(stack, mesh)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    source = {"tags": [mesh.material_tags[n] for n in P["names"]], "fwhm": P["fwhm"], "z0": P["z0"], "depth": P["depth"]}
    prob = HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, bcs if keep_line else bcs[:3], ic, source=source, **kw)
    prob.heat = heat
    return prob


def amplitudes(P, times, F1):
    return P["power"] * so.gaussian_pulse(times, P["t0"], P["w"]) / (2.0 * math.pi * math.fsum(F1))


def source_names(P):
    return [nm for nm in SOURCE_PARAMS if nm != "source.depth" or math.isfinite(P["depth"])]


def tangent_run(prob, case, P, nodes, nsteps=NSTEPS, keep_line=False, monitor_tangents=False):
    """One tangent run with the columns p_sample (k), p_sample.rho_c, the source's parameters and, with the line kept, the line's
    fwhm: (names, times, samples, tangent samples (n_steps, n_par, n_s), iters)."""
    _, _, mesh = case
    t = mesh.material_tags
    names = ["p_sample", "p_sample.rho_c"] + source_names(P) + (["fwhm"] if keep_line else [])
    times = (np.arange(nsteps) + 1) * prob.dt
    F1, Gf, Gd = prob.source_vector(), prob.source_derivative("fwhm"), prob.source_derivative("depth")
    table = coefficient_table(P["power"], P["t0"], P["w"], times, F1, Gf, Gd)
    cols = {j: {"amplitude": table[nm][:, 0], "fwhm": table[nm][:, 1], "depth": table[nm][:, 2]}
            for j, nm in enumerate(names) if nm in table}
    n = len(names)
    cond = [[t["p_sample"]]] + [[] for _ in range(n - 1)]
    cap = [[], [t["p_sample"]]] + [[] for _ in range(n - 2)]
    bnd = {n - 1: {3: prob.heat.gaussian_dfwhm}} if keep_line else None
    tv = [prob.bcs[3]] if keep_line else []
    times, s, ts, it, _ = prob.run_tangent(nsteps, nodes, conductivity=cond, capacity=cap, boundary=bnd, time_varying=tv,
                                           source=cols, source_amplitude=amplitudes(P, times, F1),
                                           **({"monitor_tangents": True} if monitor_tangents else {}))
    return names, times, s, ts, it


def primal_run(prob, P, nodes, nsteps=NSTEPS, keep_line=False):
    times = (np.arange(nsteps) + 1) * prob.dt
    return prob.run(nsteps, nodes, time_varying=[prob.bcs[3]] if keep_line else [],
                    source_amplitude=amplitudes(P, times, prob.source_vector()))
