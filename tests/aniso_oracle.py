"""Anisotropic-conductivity restatement (hf_set_anisotropy) for the CPU and GPU tests.  TEST CODE: never imported by heatflow_amd.

A cell tag may carry multipliers (m_r, m_z): its elements conduct with k_r = m_r k along r and k_z = m_z k along z, the tensor
diagonal in (z, r) and constant per element.  With grad phi_i = (b_i, c_i) / d (b_i = r_j - r_k the z-component, c_i = z_k - z_j
the r-component, oracle.heat_oracle.element_matrices) the element stiffness is

    K_ij = |K| rbar (k_z b_i b_j + k_r c_i c_j) / d^2

and the mass matrix does not change.  An element whose tag has m_r == m_z goes through oracle.heat_oracle.element_matrices with
kappa * m, as the kernel sends it through the isotropic element routine: with every multiplier 1 the matrices, and the fields of
the loops below, are bit for bit those of kappa_T_oracle.linear_fields.

On top of the matrices: the time loop of kappa_T_oracle.linear_fields for both schemes, and the steady solve with the hold load
as tests/test_steady_cpu.py and tests/test_gpu_steady.py restate them.
"""
import numpy as np
import scipy.sparse.linalg as spla

from loops_oracle import BDF2, BE, linear_loop
from oracle import heat_oracle as ho


def cell_multipliers(tags, aniso):
    """(m_r, m_z) per cell from {cell tag: (m_r, m_z)}; tags not listed are isotropic (1, 1)."""
    tags = np.asarray(tags)
    m_r, m_z = np.ones(len(tags)), np.ones(len(tags))
    for t, (a, b) in (aniso or {}).items():
        sel = tags == int(t)
        m_r[sel], m_z[sel] = float(a), float(b)
    return m_r, m_z


def element_matrices_aniso(zr, tri, rho_c, kappa, m_r, m_z):
    """Closed-form r-weighted P1 mass and stiffness with the tensor diag(k_z, k_r) = kappa diag(m_z, m_r).  (Me, Ke)."""
    zr = np.asarray(zr, dtype=np.float64)
    tri = np.asarray(tri, dtype=np.int64)
    kappa, m_r, m_z = (np.broadcast_to(np.asarray(a, dtype=np.float64), (len(tri),)) for a in (kappa, m_r, m_z))
    Me, Ke = ho.element_matrices(zr, tri, rho_c, kappa * m_r)          # right wherever m_r == m_z
    an = m_r != m_z
    if an.any():
        p = zr[tri[an]]
        z, r = p[:, :, 0], p[:, :, 1]
        d = (z[:, 1] - z[:, 0]) * (r[:, 2] - r[:, 0]) - (z[:, 2] - z[:, 0]) * (r[:, 1] - r[:, 0])
        area = 0.5 * np.abs(d)
        b = np.stack([r[:, 1] - r[:, 2], r[:, 2] - r[:, 0], r[:, 0] - r[:, 1]], axis=1)
        c = np.stack([z[:, 2] - z[:, 1], z[:, 0] - z[:, 2], z[:, 1] - z[:, 0]], axis=1)
        rbar = r.sum(axis=1) / 3.0
        k_z, k_r = (kappa * m_z)[an], (kappa * m_r)[an]
        gg = (k_z[:, None, None] * (b[:, :, None] * b[:, None, :]) + k_r[:, None, None] * (c[:, :, None] * c[:, None, :])) \
            / (d * d)[:, None, None]
        Ke[an] = (area * rbar)[:, None, None] * gg
    return Me, Ke


def element_matrices_aniso_quadrature(zr, tri, rho_c, kappa, m_r, m_z):
    """The same by numerical quadrature of the weak form int (k_z u_z v_z + k_r u_r v_r) r dx (Dunavant 6-point rule of
    oracle.heat_oracle.element_matrices_quadrature); pins the closed form, the assignment of k_r and k_z included."""
    zr = np.asarray(zr, dtype=np.float64)
    p = zr[np.asarray(tri)]
    z, r = p[:, :, 0], p[:, :, 1]
    d = (z[:, 1] - z[:, 0]) * (r[:, 2] - r[:, 0]) - (z[:, 2] - z[:, 0]) * (r[:, 1] - r[:, 0])
    area = 0.5 * np.abs(d)
    dz = np.stack([r[:, 1] - r[:, 2], r[:, 2] - r[:, 0], r[:, 0] - r[:, 1]], axis=1) / d[:, None]     # d phi_i / dz
    dr = np.stack([z[:, 2] - z[:, 1], z[:, 0] - z[:, 2], z[:, 1] - z[:, 0]], axis=1) / d[:, None]     # d phi_i / dr
    ne = len(tri)
    Me, Ke = np.zeros((ne, 3, 3)), np.zeros((ne, 3, 3))
    k_z, k_r = kappa * m_z, kappa * m_r
    for q in range(len(ho._QWTS)):
        lam = ho._QPTS[q]
        rq = r @ lam
        w = ho._QWTS[q] * area
        for i in range(3):
            for j in range(3):
                Me[:, i, j] += w * rho_c * lam[i] * lam[j] * rq
                Ke[:, i, j] += w * (k_z * dz[:, i] * dz[:, j] + k_r * dr[:, i] * dr[:, j]) * rq
    return Me, Ke


def matrices(coords, tris, tags, tag_to_k, tag_to_rc, aniso):
    """(M, K) assembled: CSR, sorted columns."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    kappa, rc = ho.cell_coefficients(np.asarray(tags), tag_to_k, tag_to_rc)
    m_r, m_z = cell_multipliers(tags, aniso)
    Me, Ke = element_matrices_aniso(coords, tris, rc, kappa, m_r, m_z)
    n = len(coords)
    return ho.assemble_csr(n, tris, Me), ho.assemble_csr(n, tris, Ke)


def operator(coords, tris, tags, tag_to_k, tag_to_rc, aniso, dtp):
    """(M, A = M + dtp K summed per element as linear_fields sums it, K)."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    kappa, rc = ho.cell_coefficients(np.asarray(tags), tag_to_k, tag_to_rc)
    m_r, m_z = cell_multipliers(tags, aniso)
    Me, Ke = element_matrices_aniso(coords, tris, rc, kappa, m_r, m_z)
    n = len(coords)
    return ho.assemble_csr(n, tris, Me), ho.assemble_csr(n, tris, Me + dtp * Ke), ho.assemble_csr(n, tris, Ke)


def aniso_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, aniso, scheme=BE):
    """Every step's field (n_steps x n): the loop of kappa_T_oracle.linear_fields on the anisotropic operator."""
    dtp = 2.0 * dt / 3.0 if scheme == BDF2 else float(dt)
    M, A, _ = operator(coords, tris, tags, tag_to_k, tag_to_rc, aniso, dtp)
    return linear_loop(M, A, bc_dofs, u0, g_all, scheme)


def steady_solve(K, dofs, g, F=None):
    """K_hat_S u = F - K[:, S] g_S on the free rows, u_S = g_S (scipy direct solve; tests/test_gpu_steady.py)."""
    dofs = np.asarray(dofs, dtype=np.int64)
    b = (np.zeros(K.shape[0]) if F is None else np.array(F, dtype=np.float64)) - K[:, dofs] @ g
    b[dofs] = g
    return spla.spsolve(ho.eliminate_dirichlet(K, dofs).tocsc(), b)


def hold_load(K, u, B):
    """(K u)_i off the transient's Dirichlet rows B, 0 on them."""
    F = K @ u
    F[np.asarray(B, dtype=np.int64)] = 0.0
    return F


def mixed_multipliers(mesh, m_r=2.0, m_z=0.25):
    """The tests' mixed case: the insulators and the sample anisotropic, every other material isotropic."""
    return {t: (m_r, m_z) for name, t in mesh.material_tags.items() if name.endswith("ins") or name == "p_sample"}


def stretched(coords, tag_to_k, tag_to_rc, s):
    """The isotropic twin of a uniform anisotropy k_r / k_z = s^2 (m_r = 1, m_z = 1 / s^2): coordinates (s z, r), k' = k / s,
    rho_c' = rho_c / s.  Substituting z' = s z in the weak form gives dz = dz' / s and u_z = s u_z', so the capacity term carries
    rho_c / s, the axial term k_z s and the radial term k_r / s - both k / s when k_r = k and k_z = k / s^2: M' = M and K' = K
    entry by entry (a power of two for s keeps the stretched coordinates exact)."""
    c = np.array(coords, dtype=np.float64)
    c[:, 0] *= s
    return c, {t: v / s for t, v in tag_to_k.items()}, {t: v / s for t, v in tag_to_rc.items()}
