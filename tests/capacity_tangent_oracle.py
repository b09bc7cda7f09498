"""Capacity-column restatement (hf_tangent_set_capacity) for the CPU and GPU tests.  TEST CODE: never imported by
heatflow_amd.

Column j carries the rho_c of a set of cell tags T_j.  With M^1_j the r-weighted mass matrix of the elements of those tags at
rho_c = 1 (un-eliminated), differentiating the step (M + dt' K) u^{n+1} = M (...) with respect to that rho_c puts

    F_j = -M^1_j w,   w = step_rate(...) of shape_tangent_oracle (both schemes, in the kernel's order of operations)

into the dt' F slot of the tangent stage.  The backend extends ShapeTangentOracleBackend (sparse LU, both set-ups, shape columns)
by tangent_set_capacity and that term in _loads.
"""
import numpy as np

from oracle import heat_oracle as ho
from shape_tangent_oracle import ShapeTangentOracleBackend, step_rate

# The relative step of the central differences in rho_c, found by tests/test_capacity_tangent_cpu.py with the rule of DESIGN.md
# 3.15 ("start at 1e-3, halve until the float64 difference is within a quarter of 1e-4 of max|s|"), and used by the GPU test too
FD_REL_STEP = {"p_sample.rho_c": 1e-3, "p_ins.cv": 1e-3, "p_sample.k+rho_c": 1e-3}


def unit_mass_matrix(coords, tris, tags, tag_set):
    """M^1 of the elements whose tag is in ``tag_set``: the oracle's element mass at rho_c = 1 there and 0 elsewhere (CSR,
    un-eliminated)."""
    tags = np.asarray(tags)
    rc = np.isin(tags, [int(t) for t in tag_set]).astype(np.float64)
    Me, _ = ho.element_matrices(coords, tris, rc, np.zeros(len(tags)))
    return ho.assemble_csr(len(coords), tris, Me)


class CapacityTangentOracleBackend(ShapeTangentOracleBackend):
    """ShapeTangentOracleBackend plus tangent_set_capacity: the recursion with the loads -M^1_j w by sparse LU, and the complete
    load of a column with the sum of absolute terms the GPU's load is held to."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._cap = {}

    def set_mesh(self, *a, **kw):
        self._cap = {}
        super().set_mesh(*a, **kw)

    def tangent_setup(self, n_par, tag_col):
        super().tangent_setup(n_par, tag_col)
        self._cap = {}

    def tangent_setup_dir(self, n_par, k=None, r=None, z=None):
        super().tangent_setup_dir(n_par, k, r, z)
        self._cap = {}

    def tangent_set_capacity(self, tag_col):
        if not self.tangent_nv:
            raise RuntimeError("tangent_set_capacity before a tangent set-up")
        cap = {}
        used = set(int(t) for t in np.unique(self.tags))
        for t, j in dict(tag_col or {}).items():
            if not 0 <= int(j) < self._npar:
                raise ValueError(f"tangent_set_capacity: tag {t} maps its rho_c to column {j} outside [-1,{self._npar})")
            if int(t) not in used:
                raise ValueError(f"tangent_set_capacity: tag {t} is not a cell tag of the mesh")
            cap.setdefault(int(j), []).append(int(t))
        self._cap = {j: unit_mass_matrix(self.coords, self.tris, self.tags, ts) for j, ts in cap.items()}
        self._reset_tangents()

    def _loads(self, mats, w):
        F, T = super()._loads(mats, w)
        for j, M1 in self._cap.items():
            F[:, j] = F[:, j] - (M1 @ w)
            T[:, j] += abs(M1) @ np.abs(w)
        return F, T

    def capacity_terms(self, j, state):
        """(M^1_j w, sum_k |M^1_jk w_k|) per row at the states (u^{n+1}, u^n, u^{n-1}): the capacity part alone."""
        w = step_rate(self.scheme, self._dt_step, *(np.asarray(s, dtype=np.float64) for s in state))
        M1 = self._cap[j]
        return M1 @ w, abs(M1) @ np.abs(w)

    def run_tangent(self, g_all, h_all=None, rtol=1e-10, atol=0.0, max_it=20000, nodes=None):
        if not self._cap or self._shape:          # (with a shape column the parent's loop already goes through _loads)
            return super().run_tangent(g_all, h_all, rtol, atol, max_it, nodes)
        # the parent's loop runs only with a shape column: an all-zero velocity on column 0 adds exact zeros to its load
        self._shape = {0: np.zeros(self.n)}
        try:
            return super().run_tangent(g_all, h_all, rtol, atol, max_it, nodes)
        finally:
            self._shape = {}


def identity_terms(prob, tag_to_k, tag_to_rc, nodes, nsteps, ic):
    """([k_t s_{k_t} ...], [c_t s_{c_t} ...]) over all cell tags of a HeatProblem, each the stacked (samples, final field): every
    tag a column of its own, the k columns and the rho_c columns in runs of at most 16 columns each, all from the state ``ic``."""
    tags = sorted(tag_to_k)
    out = []
    for kind, coef in (("conductivity", tag_to_k), ("capacity", tag_to_rc)):
        terms = []
        for lo in range(0, len(tags), 16):
            chunk = tags[lo:lo + 16]
            prob.set_state(ic)
            _, _, ts, _, _ = prob.run_tangent(nsteps, nodes, time_varying=[prob.bcs[3]], **{kind: [[t] for t in chunk]})
            terms += [coef[t] * np.concatenate([ts[:, j].ravel(), prob.tangent(j)]) for j, t in enumerate(chunk)]
        out.append(terms)
    return out
