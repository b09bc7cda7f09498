"""Shape-column restatement (hf_tangent_set_shape) for the CPU and GPU tests.  TEST CODE: never imported by
heatflow_amd.

A shape column moves the nodes along z with a nodal velocity v = dz / dtheta and keeps the triangles.  With e_a the edge opposite
vertex a (x = z, y = r), edot_a.x the difference of v over that edge and edot_a.y = 0:

    D = e_1.x e_2.y - e_1.y e_2.x,   Ddot = edot_1.x e_2.y - e_1.y edot_2.x,   delta = Ddot / D,   d = |D|
    Mdot_e = delta M_e
    Kdot_ab = -delta K_ab + rsum / (6 d) k_r (edot_a.x e_b.x + e_a.x edot_b.x),   K_ab = rsum / (6 d) (k_r e_a.x e_b.x + k_z e_a.y e_b.y)

and the column's load gets F = -Kdot u^{n+1} - Mdot w added, w = (u^{n+1} - u^n) / dt (backward Euler) or
((u^{n+1} - 4/3 u^n) + 1/3 u^{n-1}) / dt' (BDF2, dt' = 2 dt / 3, u^{-1} = u^0).  The backend extends DirTangentOracleBackend (both
schemes, the anisotropic operator, both tangent set-ups) by tangent_set_shape and the complete load.
"""
import numpy as np

from aniso_oracle import cell_multipliers, element_matrices_aniso
from bdf2_oracle import BDF2
from dir_tangent_oracle import DirTangentOracleBackend
from oracle import heat_oracle as ho


# The relative step of the central differences on moved meshes, found by tests/test_shape_tangent_cpu.py with the rule "start at
# 1e-3 of the thickness, halve until the float64 difference is within a quarter of 1e-4 of max|s|", and used by the GPU test too
FD_REL_STEP = {"p_sample.thickness": 1e-3, "p_ins.thickness": 1e-3}


def shape_element_matrices(coords, tris, rho_c, kappa, m_r, m_z, v):
    """(Mdot_e, Kdot_e), n_e x 3 x 3 each, for the nodal z-velocity ``v`` (n values)."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    ne = len(tris)
    rho_c, kappa, m_r, m_z = (np.broadcast_to(np.asarray(a, dtype=np.float64), (ne,)) for a in (rho_c, kappa, m_r, m_z))
    p, vv = coords[tris], np.asarray(v, dtype=np.float64)[tris]
    z, r = p[:, :, 0], p[:, :, 1]
    nxt, prv = [1, 2, 0], [2, 0, 1]
    ex = z[:, prv] - z[:, nxt]            # e_a = P_prev(a) - P_next(a): the edge opposite a
    ey = r[:, prv] - r[:, nxt]
    dx = vv[:, prv] - vv[:, nxt]
    D = ex[:, 1] * ey[:, 2] - ey[:, 1] * ex[:, 2]
    Dd = dx[:, 1] * ey[:, 2] - ey[:, 1] * dx[:, 2]
    delta = Dd / D
    Me, Ke = element_matrices_aniso(coords, tris, rho_c, kappa, m_r, m_z)
    fac = r.sum(axis=1) / (6.0 * np.abs(D)) * (kappa * m_r)
    sym = dx[:, :, None] * ex[:, None, :] + ex[:, :, None] * dx[:, None, :]
    return delta[:, None, None] * Me, -delta[:, None, None] * Ke + fac[:, None, None] * sym


def shape_matrices(coords, tris, tags, tag_to_k, tag_to_rc, aniso, v):
    """(Mdot, Kdot) assembled (CSR, un-eliminated) for the velocity ``v``."""
    kappa, rc = ho.cell_coefficients(np.asarray(tags), tag_to_k, tag_to_rc)
    m_r, m_z = cell_multipliers(tags, aniso)
    Md, Kd = shape_element_matrices(coords, tris, rc, kappa, m_r, m_z, v)
    n = len(coords)
    return ho.assemble_csr(n, tris, Md), ho.assemble_csr(n, tris, Kd)


def step_rate(scheme, dt, u1, un, um1):
    """w of a step, in the order of operations of the kernel's staging."""
    if scheme == BDF2:
        return ((u1 - (4.0 / 3.0) * un) + (1.0 / 3.0) * um1) / (2.0 * dt / 3.0)
    return (u1 - un) / dt


class ShapeTangentOracleBackend(DirTangentOracleBackend):
    """DirTangentOracleBackend plus tangent_set_shape: the recursion with the shape loads by sparse LU, and the complete load of
    a column with the sum of absolute terms the GPU's load is held to."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._shape = {}
        self._kept = None
        self._npar = 0

    def set_mesh(self, *a, **kw):
        self._shape, self._kept = {}, None
        super().set_mesh(*a, **kw)

    def tangent_setup(self, n_par, tag_col):
        super().tangent_setup(n_par, tag_col)
        self._shape, self._kept, self._sprev, self._npar = {}, None, None, int(n_par)

    def tangent_setup_dir(self, n_par, k=None, r=None, z=None):
        super().tangent_setup_dir(n_par, k, r, z)
        self._shape, self._kept, self._sprev, self._npar = {}, None, None, int(n_par)

    def _reset_tangents(self):
        super()._reset_tangents()
        self._kept = None

    def tangent_set_shape(self, j, vz):
        if not self.tangent_nv:
            raise RuntimeError("tangent_set_shape before a tangent set-up")
        if not 0 <= int(j) < self._npar:
            raise ValueError(f"tangent_set_shape: column {j} outside [0,{self._npar})")
        if vz is None:
            self._shape.pop(int(j), None)
        else:
            v = np.array(vz, dtype=np.float64).reshape(-1)
            if v.shape != (self.n,) or not np.all(np.isfinite(v)):
                raise ValueError("tangent_set_shape: n finite velocities expected")
            if int(j) not in self._shape and len(self._shape) == 4:
                raise ValueError("tangent_set_shape: a fifth shape column")
            self._shape[int(j)] = v
        self._reset_tangents()

    def _shape_mats(self):
        return {j: shape_matrices(self.coords, self.tris, self.tags, self.tag_to_k, self.tag_to_rc, self.aniso, v)
                for j, v in self._shape.items()}

    def _loads(self, mats, w):
        """(F, bound terms) n x nv: the complete loads and, per row, sum |Kdot_ij u_j| + sum |Mdot_ij w_j| (+ the conductivity
        part's sum |K_ij u_j| where the column has one)."""
        F = np.stack([-(self._Kj[j] @ self.u) for j in range(self.tangent_nv)], axis=1)
        T = np.stack([abs(self._Kj[j]) @ np.abs(self.u) for j in range(self.tangent_nv)], axis=1)
        for j, (Md, Kd) in mats.items():
            F[:, j] = F[:, j] - (Kd @ self.u) - (Md @ w)
            T[:, j] += abs(Kd) @ np.abs(self.u) + abs(Md) @ np.abs(w)
        return F, T

    def run_tangent(self, g_all, h_all=None, rtol=1e-10, atol=0.0, max_it=20000, nodes=None):
        if not self._shape:
            return super().run_tangent(g_all, h_all, rtol, atol, max_it, nodes)
        nv, ns = self.tangent_nv, 0 if nodes is None else len(nodes)
        nodes = None if nodes is None else np.asarray(nodes)
        nsteps = len(g_all)
        mats = self._shape_mats()
        samples, tsamples = np.empty((nsteps, ns)), np.empty((nsteps, nv, ns))
        for k, g in enumerate(g_all):
            un = self.u.copy()
            um1 = un if self._uprev is None else self._uprev.copy()
            self.step(g)
            w = step_rate(self.scheme, self._dt_step, self.u, un, um1)
            self._kept = (un, um1)
            F, _ = self._loads(mats, w)
            S_prev = self.S.copy()
            for j in range(nv):
                h = h_all[k, :, j] if h_all is not None else np.zeros(self.n_bc)
                sp = None if getattr(self, "_sprev", None) is None else self._sprev[:, j]
                b = self._rhs(self.M, self.S[:, j], sp, F[:, j])
                if self.n_bc:
                    b -= self.A_lift @ h
                    b[self.bc_dofs] = h
                self.S[:, j] = self._lu.solve(b)
            self._sprev = S_prev
            if ns:
                samples[k] = self.u[nodes]
                tsamples[k] = self.S[nodes].T
        return samples, np.ones(nsteps, dtype=np.int32), tsamples, np.ones((nsteps, nv), dtype=np.int32)

    def tangent_load_terms(self, j, state=None):
        """(F_j, bound terms of the rows) of the last step (the states kept by run_tangent; w = 0 where none was taken).
        ``state`` = (u^{n+1}, u^n, u^{n-1}) evaluates at given fields instead (the GPU's, in the GPU tests)."""
        if state is not None:
            u_keep, self.u = self.u, np.asarray(state[0], dtype=np.float64)
            try:
                w = step_rate(self.scheme, self._dt_step, self.u, np.asarray(state[1]), np.asarray(state[2]))
                F, T = self._loads(self._shape_mats(), w)
            finally:
                self.u = u_keep
            return F[:, j], T[:, j]
        w = np.zeros(self.n) if self._kept is None else step_rate(self.scheme, self._dt_step, self.u, *self._kept)
        F, T = self._loads(self._shape_mats(), w)
        return F[:, j], T[:, j]

    def tangent_load(self, j):
        return self.tangent_load_terms(j)[0]
