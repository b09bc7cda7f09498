"""Restatement of the Picard steady state under kappa(T) tables (hf_steady_picard_setup / hf_steady_picard_solve) and of the
loaded time loop under kappa(T) / rho_c(T) tables, for the CPU and GPU tests.  TEST CODE: never imported by heatflow_amd.

Steady state, with K(x) = the r-weighted stiffness at kappa_e = table_tag(T_e(x)) (kappa_T_oracle.element_kappa):
    x_0 = the start state
    sweep k = 1, 2, ...:  K_hat_S(x_{k-1}) x_k = F - K(x_{k-1})[:, S] g_S on the free rows, (x_k)_S = g_S   (direct solve)
                          change_k = max |x_k - x_{k-1}|;  stop when change_k <= picard_tol
    K(u) at the returned state u = x_k;  nl_resid = ||D^-1 (b(u) - K_hat_S(u) u)||_2 / ||D^-1 b(u)||_2, D = diag K_hat_S(u),
    b(u) = F - K(u)[:, S] g_S, b_S = g_S
Loaded loop: rhoc_T_oracle.rhoc_t_fields with b = M_k w + dt' F in every sweep.
"""
import numpy as np
import scipy.sparse.linalg as spla

from kappa_T_oracle import BDF2, BE, element_kappa
from oracle import heat_oracle as ho
from rhoc_T_oracle import operators

__all__ = ["BE", "BDF2", "stiffness", "nl_residual", "picard_steady", "loaded_fields", "rectangle_mesh"]


def stiffness(coords, tris, tags, tag_to_k, x, kappa_tables=None):
    """K(x): the r-weighted P1 stiffness with kappa_e = table_tag(T_e(x)) for a tabled tag, the constant otherwise."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    kappa = element_kappa(x, tris, tags, tag_to_k, kappa_tables or {})
    Ke = ho.element_matrices(coords, tris, np.ones(len(tris)), kappa)[1]
    return ho.assemble_csr(len(coords), tris, Ke)


def _system(K, dofs, g, F):
    b = (np.zeros(K.shape[0]) if F is None else np.array(F, dtype=np.float64)) - K[:, dofs].tocsr() @ g
    b[dofs] = g
    return ho.eliminate_dirichlet(K, dofs), b


def nl_residual(K, dofs, g, u, F=None):
    """||D^-1 (b - K_hat_S u)||_2 / ||D^-1 b||_2 of the system valued with K."""
    Khat, b = _system(K, dofs, g, F)
    d = Khat.diagonal()
    return float(np.linalg.norm((b - Khat @ u) / d) / max(np.linalg.norm(b / d), 1e-300))


def picard_steady(coords, tris, tags, tag_to_k, dofs, g, x0, kappa_tables=None, F=None, picard_tol=1e-6, max_sweeps=50):
    """The loop above.  Returns {"u", "changes" (per sweep), "sweeps", "converged", "nl_resid", "K" (valued at u)}."""
    dofs = np.asarray(dofs, dtype=np.int64)
    g = np.asarray(g, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    changes = []
    for _ in range(int(max_sweeps)):
        Khat, b = _system(stiffness(coords, tris, tags, tag_to_k, x, kappa_tables), dofs, g, F)
        xn = spla.splu(Khat.tocsc()).solve(b)
        xn[dofs] = g
        changes.append(float(np.abs(xn - x).max()))
        x = xn
        if changes[-1] <= picard_tol:
            break
    K = stiffness(coords, tris, tags, tag_to_k, x, kappa_tables)
    return {"u": x, "changes": changes, "sweeps": len(changes), "converged": changes[-1] <= picard_tol,
            "nl_resid": nl_residual(K, dofs, g, x, F), "K": K}


def loaded_fields(coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, u0, g_all, F, rhoc_tables=None, kappa_tables=None,
                  scheme=BE, picard=1):
    """Every step's field of the time loop under tables with the load term: sweep k solves
    A_k x_k = M_k w + dt' F - A_k[:, B] g on the free rows, (x_k)_B = g (rhoc_T_oracle's loop plus dt' F)."""
    bc_dofs = np.asarray(bc_dofs, dtype=np.int64)
    dtp = 2.0 * dt / 3.0 if scheme == BDF2 else float(dt)
    F = np.asarray(F, dtype=np.float64)
    u = np.array(u0, dtype=np.float64)
    up = None
    fields = []
    for g in np.asarray(g_all, dtype=np.float64):
        if scheme == BDF2:
            um1 = u if up is None else up
            w = (4.0 * u - um1) / 3.0
            x = u.copy() if up is None else 2.0 * u - up
        else:
            w = u
            x = u.copy()
        for _ in range(int(picard)):
            M, A = operators(coords, tris, tags, tag_to_k, tag_to_rc, dtp, x, kappa_tables, rhoc_tables)
            b = M @ w + dtp * F
            if len(bc_dofs):
                b -= A[:, bc_dofs].tocsr() @ g
                b[bc_dofs] = g
                A = ho.eliminate_dirichlet(A, bc_dofs)
            x = spla.splu(A.tocsc()).solve(b)
        up, u = u, x
        fields.append(u.copy())
    return np.array(fields)


def rectangle_mesh(nz, nr, L, R):
    """Structured triangulation of [0, L] x [0, R] ((z, r) coordinates): nz x nr cells, two triangles each, diagonals alternating."""
    z = np.linspace(0.0, L, nz + 1)
    r = np.linspace(0.0, R, nr + 1)
    Z, Rr = np.meshgrid(z, r, indexing="ij")
    coords = np.column_stack([Z.ravel(), Rr.ravel()])
    idx = np.arange((nz + 1) * (nr + 1)).reshape(nz + 1, nr + 1)
    tris = []
    for i in range(nz):
        for j in range(nr):
            a, b, c, d = idx[i, j], idx[i + 1, j], idx[i + 1, j + 1], idx[i, j + 1]
            tris += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return coords, np.array(tris, dtype=np.int64)
