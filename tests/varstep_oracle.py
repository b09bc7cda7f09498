"""Float64 restatement of variable time steps (hf_set_step, hf_set_step_list, hf_set_step_control) for the CPU
and GPU tests.  TEST CODE: never imported by heatflow_amd.

One step of size h after steps h_1 (the last), h_2, ... from a rest start:
    backward Euler   (M + h K) u^{n+1} = M u^n + h F
    BDF2             w = h / h_1 (1 from rest),  dt' = h (1+w)/(1+2w),  (M + dt' K) u^{n+1} = M (a u^n - b u^{n-1}) + dt' F
with lifting and set_bc as in the constant-step loops, one scipy LU per distinct dt', F = F0 + p F1 (load and source), and under
tables the lagged scheme of loops_oracle.table_loop with the evaluation state u^n, or (1+w) u^n - w u^{n-1} under BDF2 with a
history.  The coefficient formulas, the predictor weights and the estimator's constant are heatflow_amd.stepping's - the
formulas the driver of the GPU path uses; what is restated here is the loop around them.
"""
import copy
import functools
import math

import numpy as np
import scipy.sparse.linalg as spla

from aniso_oracle import operator as aniso_operator
from bdf2_oracle import BDF2, BDF2OracleBackend
from oracle import heat_oracle as ho
from rhoc_T_oracle import operators
from source_oracle import source_vector

from heatflow_amd import stepping


class VarstepOracleBackend(BDF2OracleBackend):
    """The scipy stand-in for HeatflowHIP with the variable-step calls: set_step, set_step_list, set_step_control, step_error,
    step_reject, step_info; load, source, anisotropy and lagged tables as the library's single-run loop has them."""

    def __init__(self, device_id=0):
        super().__init__(device_id)
        self._aniso, self._ktab, self._ctab, self._picard = {}, {}, {}, 1
        self._F1, self._amps, self._amp_next = None, [], 0
        self._list, self._list_next, self._dt_next = [], 0, None
        self._control = False
        self._lus = {}
        self._rest()
        self.revaluations = 0

    # -- set-up ---------------------------------------------------------------------------
    def _rest(self):
        self._t, self._steps, self._hist, self._undo = 0.0, [], [], None

    def set_anisotropy(self, multipliers):
        self._aniso = {int(t): (float(v[0]), float(v[1])) for t, v in (multipliers or {}).items()}

    def set_aniso_tables(self, on):
        raise NotImplementedError("VarstepOracleBackend: no tables on anisotropic tags")

    def set_kappa_tables(self, tables, picard=1):
        self._ktab = {int(t): v for t, v in (tables or {}).items()}
        if self._ktab:
            self._picard = int(picard)

    def set_rhoc_tables(self, tables):
        self._ctab = {int(t): v for t, v in (tables or {}).items()}

    def set_picard(self, sweeps):
        self._picard = int(sweeps)

    def set_source(self, tags, fwhm=1.0, z0=0.0, depth=float("inf")):
        self._F1 = None if tags is None or len(tags) == 0 else source_vector(self.coords, self.tris, self.tags, [int(t) for t in tags],
                                                                             fwhm, z0, depth)[0]

    def get_source(self):
        return self._F1.copy()

    def set_source_amplitudes(self, p):
        self._amps, self._amp_next = [float(x) for x in np.ravel([] if p is None else p)], 0

    def _operators(self, dtp, x):
        """(M, A = M + dtp K), not eliminated, at the state x (which matters under tables only)."""
        if self._aniso:
            if self._ktab or self._ctab:
                raise NotImplementedError
            M, A, _ = aniso_operator(self.coords, self.tris, self.tags, self.tag_to_k, self.tag_to_rc, self._aniso, dtp)
            return M, A
        return operators(self.coords, self.tris, self.tags, self.tag_to_k, self.tag_to_rc, dtp, x, self._ktab, self._ctab)

    def _factor(self, dtp, x):
        """(M, lifting columns, LU of the eliminated A) at dt'; without tables one factorisation per distinct dt'."""
        tabled = bool(self._ktab or self._ctab)
        key = float(dtp)
        if not tabled and key in self._lus:
            return self._lus[key]
        M, A = self._operators(dtp, x)
        lift = A[:, self.bc_dofs].tocsr() if self.n_bc else None
        lu = spla.splu((ho.eliminate_dirichlet(A, self.bc_dofs) if self.n_bc else A).tocsc())
        if not tabled:
            self._lus[key] = (M, lift, lu)
        return M, lift, lu

    def assemble(self, dt, mode=0):
        self._dt_step, self._dt_next = float(dt), float(dt)
        self._order = 2 if self.scheme == BDF2 else 1
        self._lus = {}
        self._dt = self._dt_held = stepping.effective_step(self._order, float(dt))
        self.M, self.A = self._operators(self._dt, self.u)
        self.nnz = self.A.nnz
        self._list, self._list_next = [], 0
        self._uprev = None
        self._rest()
        self.assemble_calls += 1

    def set_state(self, u):
        self.u = np.array(u, dtype=np.float64).copy()
        self._uprev = None
        self._rest()

    # -- the variable-step calls ---------------------------------------------------------------
    def set_step(self, dt):
        dt = float(dt)
        if not (dt > 0.0 and np.isfinite(dt)):
            raise ValueError("hf_set_step: dt must be positive and finite")
        if self._order == 2 and self._uprev is not None and dt / self._steps[-1] > stepping.BDF2_MAX_RATIO:
            raise ValueError("hf_set_step: the ratio exceeds 1 + sqrt 2")
        self._dt_next, self._list, self._list_next = dt, [], 0

    def set_step_list(self, dts):
        d = [float(x) for x in np.ravel(dts)]
        if any(not (x > 0.0 and np.isfinite(x)) for x in d):
            raise ValueError("hf_set_step_list: entries must be positive and finite")
        self._list, self._list_next = d, 0

    def set_step_control(self, on=True):
        if on and self._steps:
            raise RuntimeError("hf_set_step_control: switched on at rest only")
        self._control = bool(on)
        self._undo = None

    def step_info(self):
        return {"t": self._t, "dt_last": self._steps[-1] if self._steps else 0.0,
                "dt_eff": self._dt_last_eff if self._steps else 0.0, "revaluations": self.revaluations}

    def step(self, g, rtol=1e-10, atol=0.0, max_it=20000):
        if self._list:
            if self._list_next >= len(self._list):
                raise RuntimeError("the step list has 0 entries left")
            h = self._list[self._list_next]
        else:
            h = self._dt_next
        bdf2 = self._order == 2
        omega = h / self._steps[-1] if bdf2 and self._uprev is not None else 1.0
        if omega > stepping.BDF2_MAX_RATIO:
            raise ValueError("the ratio exceeds 1 + sqrt 2")
        undo = dict(u=self.u, uprev=self._uprev, t=self._t, steps=list(self._steps), hist=list(self._hist),
                    amp_next=self._amp_next, list_next=self._list_next, eff=getattr(self, "_dt_last_eff", 0.0))
        if self._list:
            self._list_next += 1
        dtp = stepping.effective_step(self._order, h, omega)
        if dtp != self._dt_held:
            self.revaluations += 1
            self._dt_held = dtp
        u, um1 = self.u, self.u if self._uprev is None else self._uprev
        if bdf2:
            a, b, _ = stepping.bdf2_coefficients(omega) if omega != 1.0 else (4.0 / 3.0, 1.0 / 3.0, None)
            w = (4.0 * u - um1) / 3.0 if omega == 1.0 else a * u - b * um1
            x = u.copy() if self._uprev is None else (1.0 + omega) * u - omega * um1
        else:
            w, x = u, u.copy()
        F = None if self._load is None else self._load.copy()
        if self._F1 is not None:
            p = self._amps[self._amp_next] if self._amps else 0.0
            if self._amps:
                self._amp_next += 1
            F = p * self._F1 if F is None else F + p * self._F1
        g = np.asarray(g, dtype=np.float64)
        tabled = bool(self._ktab or self._ctab)
        for _ in range(self._picard if tabled else 1):
            M, lift, lu = self._factor(dtp, x)
            rhs = M @ w if F is None else M @ w + dtp * F
            if self.n_bc:
                rhs -= lift @ g
                rhs[self.bc_dofs] = g
            x = lu.solve(rhs)
        self._hist = ([u] + self._hist)[:3]             # u^n, u^{n-1}, u^{n-2} of the step just taken
        self._uprev, self.u = u, x
        self._steps.append(h)
        self._t += h
        self._dt_last_eff = dtp
        self._undo = undo if self._control else None
        return 1, 0.0

    def step_estimate(self):
        """The estimate c (u - w0 h0 - w1 h1 - w2 h2) of the step taken last at every node, and the magnitude
        c (|u| + sum_k |w_k h_k|) its rounding bound is stated against."""
        d0, d1, d2 = stepping.history_steps(self._steps)
        hs = list(self._hist) + [self._hist[-1]] * (3 - len(self._hist))       # missing history: the rest state
        wts = stepping.predictor_weights(self._order, d0, d1, d2)
        c = stepping.estimator_constant(self._order, d0, d1, d2)
        e = self.u.copy()
        mag = np.abs(self.u)
        for wk, hk in zip(wts, hs):
            e = e - wk * hk
            mag = mag + np.abs(wk * hk)
        return c * e, c * mag

    def step_error(self, atol=1.0, rtol=0.0):
        e, _ = self.step_estimate()
        free = np.ones(self.n, dtype=bool)
        free[self.bc_dofs] = False
        return float(np.max(np.abs(e[free]) / (atol + rtol * np.abs(self.u[free]))))

    def step_reject(self):
        if not self._control or self._undo is None:
            raise RuntimeError("hf_step_reject: no step to undo")
        s = self._undo
        self.u, self._uprev, self._t, self._steps, self._hist = s["u"], s["uprev"], s["t"], s["steps"], s["hist"]
        self._amp_next, self._list_next, self._dt_last_eff = s["amp_next"], s["list_next"], s["eff"]
        self._undo = None


def pulse(t, t0=1.5e-6, fwhm=1.0e-6):
    """The smooth drive of the adaptive tests: a Gaussian in time, peak 1 at t0."""
    return np.exp(-4.0 * np.log(2.0) * (np.asarray(t, dtype=np.float64) - t0) ** 2 / (fwhm * fwhm))


# ---- shared set-up of tests/test_varstep_cpu.py and tests/test_gpu_varstep.py --------------------------------------------------
RATIOS = (1, 0.5, 2, 1.7, 0.3, 1, 1, 2.4, 0.6, 1.2, 0.25, 2)
CASES = {"with_diamond": "geballe_with_diamond", "no_diamond": "geballe_no_diamond"}


@functools.lru_cache(maxsize=None)
def small(which):
    """The 8x-coarsened stock cases.  With diamonds the stock step (7.5e-8 s) would end the 9.2-step list at 0.7 us, before the
    heating curve has risen by more than a kelvin; at 25 steps over the 7.5 us (dt = 3e-7 s) the list ends at 2.8 us."""
    cfg, stack, mesh = _build_case(CASES[which], 8.0)
    if which == "with_diamond":
        cfg = copy.deepcopy(cfg)
        cfg["timing"]["num_steps"] = 25
    return cfg, stack, mesh


def step_list(dt):
    return dt * np.cumprod(RATIOS)



def _build_case(name, scale):
    from conftest import build_case

    return build_case(name, scale)


class SmoothPulse:
    """The heated line of the issue's prototype: a Gaussian in time (FWHM 1 us, centred at 1.5 us, 500 K) times the reference's
    Gaussian in r."""

    def __init__(self, ic, fwhm_r, rise=500.0):
        self.ic, self.rise, self.coeff = float(ic), float(rise), -4.0 * math.log(2.0) / float(fwhm_r) ** 2

    def gaussian(self, x, y, t):
        return self.ic + self.rise * float(pulse(t)) * np.exp(self.coeff * np.asarray(y) ** 2)


def smooth_problem(case, backend=None, num_steps=100, **kw):
    cfg, stack, mesh = case
    c = copy.deepcopy(cfg)
    c["timing"]["t_final"] = 3.0e-5
    c["timing"]["num_steps"] = int(num_steps)
    from helpers import make_problem

    prob = make_problem(c, stack, mesh, backend=backend, **kw)
    prob.bcs[3]._value = SmoothPulse(float(cfg["heating"]["ic_temp"]), float(cfg["heating"]["fwhm"])).gaussian
    return prob


def oside_node(case):
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    return nearest_nodes(case[2].coords, [get_watcher_points(case[0])["oside"]])


@functools.lru_cache(maxsize=None)
def smooth_references():
    """o-side curves of the restatement under the smooth pulse, BDF2, 30 us: 6400 fixed steps (the reference) and the error of
    800 fixed steps against it."""
    case = small("with_diamond")
    node = oside_node(case)
    out = {}
    for n in (6400, 800):
        prob = smooth_problem(case, backend=VarstepOracleBackend(), num_steps=n, scheme="bdf2")
        t, s, _ = prob.run(n, watcher_nodes=node, time_varying=[prob.bcs[3]])
        out[n] = (t, s[:, 0])
    err800 = float(np.abs(out[800][1] - out[6400][1][7::8]).max())
    return out[6400], err800
