"""Float64 restatement of the volumetric source (hf_set_source) and of the time loop with its per-step amplitude, for the CPU
and GPU tests of laser-power heating.  TEST CODE: never imported by heatflow_amd.

    s(z, r) = exp(-(c r^2 + |z - z0| / depth)),  c = 4 ln2 / fwhm^2   (depth = inf: the second term is 0)
    F1_i    = sum over e at i with tag(e) listed, sum over j in e, of (M_e at rho_c = 1)_ij s(z_j, r_j)
    step    A' u^{n+1} = M w + dt' (F0 + p_{n+1} F1) - lifting, set_bc;  w = u^n, dt' = dt (backward Euler),
            w = (4 u^n - u^{n-1}) / 3, dt' = 2 dt / 3 (BDF2, u^{-1} = u^0)
built on oracle.heat_oracle's element matrices, assembly and elimination; with tables the operators per sweep are
rhoc_T_oracle.operators'.  The argument of exp is formed as the device forms it (the two constants first, then one product and
one sum per term), so the restated s differs from the device's only by the exp routine itself.
"""
import math

import numpy as np
import scipy.sparse.linalg as spla

from oracle import heat_oracle as ho
from rhoc_T_oracle import operators

BE, BDF2 = 0, 1


def source_shape(coords, fwhm, z0, depth):
    """s at every node."""
    zr = np.asarray(coords, dtype=np.float64)
    c_r = 4.0 * math.log(2.0) / (fwhm * fwhm)
    inv_depth = 0.0 if math.isinf(depth) else 1.0 / depth
    x = c_r * (zr[:, 1] * zr[:, 1]) + np.abs(zr[:, 0] - z0) * inv_depth
    return np.exp(-x)


def absorbing_mass(coords, tris, tags, absorbing):
    """The r-weighted P1 mass matrix at rho_c = 1 of the elements whose tag is in ``absorbing``, zero elsewhere (CSR)."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    mask = np.isin(np.asarray(tags), np.asarray(list(absorbing))).astype(np.float64)
    Me, _ = ho.element_matrices(coords, tris, mask, np.zeros(len(tris)))
    return ho.assemble_csr(len(coords), tris, Me)


def source_vector(coords, tris, tags, absorbing, fwhm, z0, depth=math.inf):
    """(F1, scale): F1 = M1 s and scale_i = sum_j |M1_ij| s_j, the magnitude a rounding bound on F1_i is stated against."""
    M1 = absorbing_mass(coords, tris, tags, absorbing)
    s = source_shape(coords, fwhm, z0, depth)
    return M1 @ s, abs(M1) @ s


def sourced_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, F1, amps, load=None, scheme=BE,
                   kappa_tables=None, rhoc_tables=None, picard=1):
    """Every step's field (n_steps x n) of the loop with the source F1 at the amplitudes ``amps`` and the constant load ``load``.
    Without tables one factorisation serves the run; with tables every Picard sweep re-values M and A at the latest iterate."""
    bc_dofs = np.asarray(bc_dofs, dtype=np.int64)
    dtp = 2.0 * dt / 3.0 if scheme == BDF2 else float(dt)
    tabled = bool(kappa_tables) or bool(rhoc_tables)
    u = np.array(u0, dtype=np.float64)
    up = None
    F0 = np.zeros(len(u)) if load is None else np.asarray(load, dtype=np.float64)
    F1 = np.asarray(F1, dtype=np.float64)
    if not tabled:
        M, A = operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, u)
        lift = A[:, bc_dofs].tocsr() if len(bc_dofs) else None
        lu = spla.splu((ho.eliminate_dirichlet(A, bc_dofs) if len(bc_dofs) else A).tocsc())
    fields = []
    for g, p in zip(np.asarray(g_all, dtype=np.float64), np.asarray(amps, dtype=np.float64)):
        if scheme == BDF2:
            w = (4.0 * u - (u if up is None else up)) / 3.0
            x = u.copy() if up is None else 2.0 * u - up
        else:
            w = u
            x = u.copy()
        f = dtp * (F0 + p * F1)
        if not tabled:
            b = M @ w + f
            if len(bc_dofs):
                b -= lift @ g
                b[bc_dofs] = g
            x = lu.solve(b)
        else:
            for _ in range(int(picard)):
                Mk, Ak = operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, x, kappa_tables, rhoc_tables)
                b = Mk @ w + f
                if len(bc_dofs):
                    b -= Ak[:, bc_dofs].tocsr() @ g
                    b[bc_dofs] = g
                    Ak = ho.eliminate_dirichlet(Ak, bc_dofs)
                x = spla.splu(Ak.tocsc()).solve(b)
        up, u = u, x
        fields.append(u.copy())
    return np.array(fields)


def gaussian_pulse(times, t0, fwhm):
    """exp(-4 ln2 (t - t0)^2 / fwhm^2): peak 1 at t0."""
    t = np.asarray(times, dtype=np.float64)
    return np.exp(-4.0 * math.log(2.0) * (t - t0) ** 2 / (fwhm * fwhm))


def peak_density(power, F1):
    """W -> W/m^3: p with 2 pi p sum(F1) = power."""
    return power / (2.0 * math.pi * math.fsum(F1))


# ---- a high-order reference for int s phi_i r over the absorbing elements (the true s, not its interpolant) --------------------
def _subdivide(p, levels):
    """The 4^levels congruent sub-triangles of the triangles p (m, 3, 2)."""
    for _ in range(levels):
        a, b, c = p[:, 0], p[:, 1], p[:, 2]
        ab, bc, ca = 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a)
        p = np.concatenate([np.stack(t, axis=1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    return p


def quadrature_load(coords, tris, tags, absorbing, shape, levels=3):
    """int s phi_i r dz dr over the absorbing elements by the degree-4 Dunavant rule on 4^levels sub-triangles of every element;
    ``shape(z, r)`` is the exact s."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    out = np.zeros(len(coords))
    for e in np.nonzero(np.isin(np.asarray(tags), np.asarray(list(absorbing))))[0]:
        P = coords[tris[e]]                                   # (3, 2)
        T = np.array([[P[1, 0] - P[0, 0], P[2, 0] - P[0, 0]], [P[1, 1] - P[0, 1], P[2, 1] - P[0, 1]]])
        Tinv = np.linalg.inv(T)
        sub = _subdivide(P[None], levels)                     # (m, 3, 2)
        d = (sub[:, 1, 0] - sub[:, 0, 0]) * (sub[:, 2, 1] - sub[:, 0, 1]) - (sub[:, 2, 0] - sub[:, 0, 0]) * (sub[:, 1, 1] - sub[:, 0, 1])
        area = 0.5 * np.abs(d)
        for lam, wq in zip(ho._QPTS, ho._QWTS):
            x = np.einsum("k,mkc->mc", lam, sub)              # quadrature points (m, 2)
            l12 = (x - P[0]) @ Tinv.T                          # barycentric coordinates 1, 2 in the parent element
            phi = np.stack([1.0 - l12[:, 0] - l12[:, 1], l12[:, 0], l12[:, 1]], axis=1)
            wgt = wq * area * shape(x[:, 0], x[:, 1]) * x[:, 1]
            out[tris[e]] += phi.T @ wgt
    return out
