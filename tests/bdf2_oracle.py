"""BDF2 restatement of the time loop (hf_set_time_scheme(HF_TIME_BDF2)) for the CPU and GPU tests of the time scheme.

Constant-step BDF2, (3/2 M + dt K) u^{n+1} = 2 M u^n - 1/2 M u^{n-1} + dt F, divided by 3/2:
    A' u^{n+1} = M (4/3 u^n - 1/3 u^{n-1}) + dt' F,   A' = M + dt' K,   dt' = 2 dt / 3,
with lifting and set_bc as in backward Euler, and u^{-1} = u^0 (a start at rest).  TEST CODE: never imported by heatflow_amd.
"""
from unittest import mock

import numpy as np

from oracle import heat_oracle as ho
from test_tangent_cpu import TangentOracleBackend

BE, BDF2 = 0, 1


class BDF2OracleSolver(ho.OracleSolver):
    """OracleSolver stepping with BDF2: assembled at 2 dt / 3, right-hand side M (4/3 u^n - 1/3 u^{n-1})."""

    def __init__(self, coords, tris, tags, tag_to_k, tag_to_rho_cv, dt, bcs, u0):
        super().__init__(coords, tris, tags, tag_to_k, tag_to_rho_cv, 2.0 * dt / 3.0, bcs, u0)
        self.u_prev = self.u.copy()

    def rhs(self, g):
        b = self.M @ ((4.0 * self.u - self.u_prev) / 3.0)
        b -= self.A_lift @ g
        b[self.bc_dofs] = g
        return b

    def step(self, t):
        b = self.rhs(self.bc_values(t))
        self.u_prev, self.u = self.u, self.factor().solve(b)
        return self.u


def reference_run(cfg, mesh, num_steps, watcher_nodes=None, scheme=BDF2, keep_fields=False):
    """ho.run_reference_algorithm at ``num_steps`` steps over the configured t_final, with the BDF2 solver (or backward Euler)."""
    from conftest import HEATING_CSV

    c = dict(cfg, timing=dict(cfg["timing"], num_steps=int(num_steps)))
    solver = BDF2OracleSolver if scheme == BDF2 else ho.OracleSolver
    with mock.patch.object(ho, "OracleSolver", solver):
        return ho.run_reference_algorithm(c, mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, HEATING_CSV,
                                          num_steps=num_steps, keep_fields=keep_fields, watcher_nodes=watcher_nodes)


class BDF2OracleBackend(TangentOracleBackend):
    """The scipy stand-in for HeatflowHIP with hf_set_time_scheme: single runs (with an optional load), the batched loop and
    tangent runs in either scheme, history u^{n-1} reset to u^n wherever the library resets it."""

    scheme = BE
    _uprev = None
    _load = None

    def set_time_scheme(self, scheme):
        scheme = {"backward_euler": BE, "bdf2": BDF2}.get(scheme, scheme)
        if scheme not in (BE, BDF2):
            raise ValueError(f"unknown scheme {scheme}")
        self.scheme = int(scheme)
        self.set_time_scheme_calls = getattr(self, "set_time_scheme_calls", 0) + 1

    def assemble(self, dt, mode=0):
        self._dt_step = dt
        super().assemble(2.0 * dt / 3.0 if self.scheme == BDF2 else dt, mode)
        self._uprev = None

    def set_state(self, u):
        super().set_state(u)
        self._uprev = None

    def set_load(self, F):
        self._load = None if F is None else np.array(F, dtype=np.float64)

    def _rhs(self, M, u, uprev, F):
        if self.scheme == BDF2:
            b = M @ ((4.0 * u - (u if uprev is None else uprev)) / 3.0)
        else:
            b = M @ u
        return b if F is None else b + self._dt * F

    def step(self, g, rtol=1e-10, atol=0.0, max_it=20000):
        b = self._rhs(self.M, self.u, self._uprev, self._load)
        if self.n_bc:
            b -= self.A_lift @ g
            b[self.bc_dofs] = g
        self._uprev, self.u = self.u, self._lu.solve(b)
        return 1, 0.0

    def batch_set_affine(self, tags, delta):
        ref, tagset = dict(self.tag_to_k), {int(x) for x in tags}
        for j, d in enumerate(delta):
            self.tag_to_k = {t: (k + float(d) if t in tagset else k) for t, k in ref.items()}
            self.assemble(self._dt_step)
            self.batch_load_column(j)
        self.tag_to_k = ref
        self.assemble(self._dt_step)

    def batch_set_state(self, j, u):
        super().batch_set_state(j, u)
        self._bcols[j]["uprev"] = None

    def batch_run(self, g_all, rtol=1e-10, atol=0.0, max_it=20000, nodes=None, flux_nodes=None, flux_components=2,
                  flux_rtol=None, flux_max_it=5000):
        if flux_nodes is not None or self.scheme == BE:
            if self.scheme == BDF2:
                raise NotImplementedError("BDF2OracleBackend: no batched flux projection")
            return super().batch_run(g_all, rtol, atol, max_it, nodes, flux_nodes, flux_components, flux_rtol, flux_max_it)
        nsteps, _, nv = g_all.shape
        ns = 0 if nodes is None else len(nodes)
        samples = np.empty((nsteps, nv, ns))
        for s in range(nsteps):
            for j, col in enumerate(self._bcols):
                b = self._rhs(col["M"], col["u"], col.get("uprev"), None)
                if self.n_bc:
                    g = np.ascontiguousarray(g_all[s, :, j])
                    b -= col["lift"] @ g
                    b[self.bc_dofs] = g
                col["uprev"], col["u"] = col["u"], col["lu"].solve(b)
                if ns:
                    samples[s, j] = col["u"][np.asarray(nodes)]
        return samples, np.ones((nsteps, nv), dtype=np.int32)

    def _reset_tangents(self):
        super()._reset_tangents()
        self._sprev = None

    def run_tangent(self, g_all, h_all=None, rtol=1e-10, atol=0.0, max_it=20000, nodes=None):
        nv, ns = self.tangent_nv, 0 if nodes is None else len(nodes)
        nodes = None if nodes is None else np.asarray(nodes)
        nsteps = len(g_all)
        samples, tsamples = np.empty((nsteps, ns)), np.empty((nsteps, nv, ns))
        for k, g in enumerate(g_all):
            self.step(g)
            S_prev = self.S.copy()
            for j in range(nv):
                h = h_all[k, :, j] if h_all is not None else np.zeros(self.n_bc)
                sp = None if getattr(self, "_sprev", None) is None else self._sprev[:, j]
                b = self._rhs(self.M, self.S[:, j], sp, -(self._Kj[j] @ self.u))
                if self.n_bc:
                    b -= self.A_lift @ h
                    b[self.bc_dofs] = h
                self.S[:, j] = self._lu.solve(b)
            self._sprev = S_prev
            if ns:
                samples[k] = self.u[nodes]
                tsamples[k] = self.S[nodes].T
        return samples, np.ones(nsteps, dtype=np.int32), tsamples, np.ones((nsteps, nv), dtype=np.int32)


def bdf2_fields(M, K, dt, bc_dofs, u0, g_all, load=None, u_prev=None):
    """Every step's field of the BDF2 loop from scipy matrices (M, the r-weighted stiffness K un-eliminated), the step dt,
    the Dirichlet dofs, the start u0 (history u_prev, default u0 = a rest start), g_all (n_steps x n_bc) and a load F."""
    import scipy.sparse.linalg as spla

    dtp = 2.0 * dt / 3.0
    A = (M + dtp * K).tocsr()
    Ahat = ho.eliminate_dirichlet(A, bc_dofs) if len(bc_dofs) else A
    lift = A[:, bc_dofs].tocsr() if len(bc_dofs) else None
    lu = spla.splu(Ahat.tocsc())
    u = np.array(u0, dtype=np.float64)
    up = u.copy() if u_prev is None else np.array(u_prev, dtype=np.float64)
    out = []
    for g in g_all:
        b = M @ ((4.0 * u - up) / 3.0)
        if load is not None:
            b = b + dtp * load
        if len(bc_dofs):
            b -= lift @ g
            b[bc_dofs] = g
        up, u = u, lu.solve(b)
        out.append(u.copy())
    return np.array(out)
