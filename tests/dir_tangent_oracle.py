"""Directional tangent restatement (hf_tangent_setup_dir / hf_tangent_load) for the CPU and GPU tests.  TEST CODE: never imported
by heatflow_amd.

Per element K_e = k_r K_e^r + k_z K_e^z with k_r = m_r kappa, k_z = m_z kappa, so the time step is affine in k_r and k_z of every
tag and the tangent recursion of test_tangent_cpu.TangentOracleBackend holds with the loads

    k_r of tag t:    F = -K_t^r u        k_z of tag t:    F = -K_t^z u        kappa of tag t:    F = -(m_r K_t^r + m_z K_t^z) u

K_t^r and K_t^z are aniso_oracle.element_matrices_aniso at kappa = 1 with the multipliers (1, 0) and (0, 1), summed over the
tag's elements.  The operator is the anisotropic one of aniso_oracle.operator, in either time scheme (bdf2_oracle).
"""
import numpy as np
import scipy.sparse.linalg as spla

from aniso_oracle import element_matrices_aniso, operator
from bdf2_oracle import BDF2, BDF2OracleBackend
from oracle import heat_oracle as ho


def directional_element_matrices(coords, tris):
    """(Ke_r, Ke_z): the element stiffness at unit k_r alone and at unit k_z alone, n_e x 3 x 3 each."""
    ne = len(tris)
    zero, one = np.zeros(ne), np.ones(ne)
    return (element_matrices_aniso(coords, tris, zero, one, one, zero)[1],
            element_matrices_aniso(coords, tris, zero, one, zero, one)[1])


def column_weights(tags, aniso, n_par, k=None, r=None, z=None):
    """Per column j the per-element weights (w_r, w_z) of K^r and K^z: ``k`` / ``r`` / ``z`` = {cell tag: column}; a kappa
    column weighs the directions with the tag's multipliers {cell tag: (m_r, m_z)} of ``aniso`` (1, 1 where not listed)."""
    tags = np.asarray(tags)
    w = np.zeros((n_par, 2, len(tags)))
    for t, j in (k or {}).items():
        m_r, m_z = (aniso or {}).get(int(t), (1.0, 1.0))
        w[j, 0, tags == int(t)] += m_r
        w[j, 1, tags == int(t)] += m_z
    for t, j in (r or {}).items():
        w[j, 0, tags == int(t)] += 1.0
    for t, j in (z or {}).items():
        w[j, 1, tags == int(t)] += 1.0
    return w


class DirTangentOracleBackend(BDF2OracleBackend):
    """BDF2OracleBackend on the anisotropic operator (set_anisotropy) with tangent_setup_dir and tangent_load."""

    aniso = None

    def set_mesh(self, *a, **kw):                 # hf_set_mesh clears the multipliers and removes a tangent set-up
        self.aniso = None
        self.tangent_nv = 0
        super().set_mesh(*a, **kw)

    def set_anisotropy(self, multipliers):        # removes a tangent set-up, as the library does
        self.aniso = {int(t): (float(v[0]), float(v[1])) for t, v in dict(multipliers or {}).items()}
        self.tangent_nv = 0

    def assemble(self, dt, mode=0):
        self._dt_step = dt
        self._dt = 2.0 * dt / 3.0 if self.scheme == BDF2 else dt
        self.M, self.A, self.K = operator(self.coords, self.tris, self.tags, self.tag_to_k, self.tag_to_rc, self.aniso, self._dt)
        self.nnz = self.A.nnz
        self.Ahat = ho.eliminate_dirichlet(self.A, self.bc_dofs) if self.n_bc else self.A
        self.A_lift = self.A[:, self.bc_dofs].tocsr() if self.n_bc else None
        self._lu = spla.splu(self.Ahat.tocsc())
        self.assemble_calls += 1
        self._uprev = None
        self._reset_tangents()

    def tangent_setup_dir(self, n_par, k=None, r=None, z=None):
        if not 1 <= n_par <= 16:
            raise ValueError("n_par outside 1..16")
        k, r, z = dict(k or {}), dict(r or {}), dict(z or {})
        if not (k or r or z):
            raise ValueError("tangent_setup_dir: no column")
        both = set(k) & (set(r) | set(z))
        if both:
            raise ValueError(f"tangent_setup_dir: tag {sorted(both)[0]} has a kappa column and a directional one")
        self.tangent_nv = next(v for v in (2, 4, 8, 16) if v >= n_par)
        Ke_r, Ke_z = directional_element_matrices(self.coords, self.tris)
        w = column_weights(self.tags, self.aniso, self.tangent_nv, k, r, z)
        self._Kj = [ho.assemble_csr(self.n, self.tris, w[j, 0][:, None, None] * Ke_r + w[j, 1][:, None, None] * Ke_z)
                    for j in range(self.tangent_nv)]
        self.S = np.zeros((self.n, self.tangent_nv))
        self._sprev = None

    def tangent_load(self, j):
        return -(self._Kj[j] @ self.u)
