"""The three loops of the float64 restatements, each once: the time loop under tables, the factor-once time loop and the Picard
steady state.  TEST CODE: never imported by heatflow_amd.

The callers (rhoc_T_oracle, aniso_T_oracle, steady_picard_oracle, kappa_T_oracle, aniso_oracle) keep their operator builders to
themselves and hand them in as closures: the tests assert that those builders agree bit for bit in the degenerate cases, which
means something only while they are independent code.  The loops here were compared with the copies they replace by
np.array_equal on every returned array (profiles/oracle_loops_equal.txt).
"""
import numpy as np
import scipy.sparse.linalg as spla

from oracle import heat_oracle as ho

BE, BDF2 = 0, 1


def table_loop(operators_at, dt, bc_dofs, u0, g_all, scheme, picard, F=None):
    """The time loop under tables, with dt' the assembled step (dt, or 2 dt / 3 under BDF2):
        u* = u^n (backward Euler), 2 u^n - u^{n-1} (BDF2 once a history exists, else u^n)
        w  = u^n (BDF2: (4 u^n - u^{n-1}) / 3, u^{n-1} = u^n without a history)
        x_0 = u*;  sweep k = 1..p:  (M_k, A_k) = operators_at(dt', x_{k-1}), not eliminated,
                   A_k x_k = M_k w + dt' F - A_k[:, B] g on the free rows,  (x_k)_B = g
        u^{n+1} = x_p;  the Picard change = max |x_p - x_{p-1}|
    Returns every step's field (n_steps x n) and the Picard change of every step."""
    bc_dofs = np.asarray(bc_dofs, dtype=np.int64)
    dtp = 2.0 * dt / 3.0 if scheme == BDF2 else float(dt)
    if F is not None:
        F = np.asarray(F, dtype=np.float64)
    u = np.array(u0, dtype=np.float64)
    up = None
    fields, changes = [], []
    for g in np.asarray(g_all, dtype=np.float64):
        if scheme == BDF2:
            um1 = u if up is None else up
            w = (4.0 * u - um1) / 3.0
            x = u.copy() if up is None else 2.0 * u - up
        else:
            w = u
            x = u.copy()
        change = 0.0
        for _ in range(int(picard)):
            M, A = operators_at(dtp, x)
            b = M @ w if F is None else M @ w + dtp * F
            if len(bc_dofs):
                b -= A[:, bc_dofs].tocsr() @ g
                b[bc_dofs] = g
                A = ho.eliminate_dirichlet(A, bc_dofs)
            xn = spla.splu(A.tocsc()).solve(b)
            change = float(np.abs(xn - x).max())
            x = xn
        up, u = u, x
        fields.append(u.copy())
        changes.append(change)
    return np.array(fields), np.array(changes)


def linear_loop(M, A, bc_dofs, u0, g_all, scheme):
    """The time loop with constant operators (M, A = M + dt' K, not eliminated): one factorisation; BDF2 from a rest start.
    Returns every step's field (n_steps x n)."""
    bc_dofs = np.asarray(bc_dofs, dtype=np.int64)
    Ahat = ho.eliminate_dirichlet(A, bc_dofs)
    lift = A[:, bc_dofs].tocsr()
    lu = spla.splu(Ahat.tocsc())
    u = np.array(u0, dtype=np.float64)
    up = u.copy()
    out = []
    for g in np.asarray(g_all, dtype=np.float64):
        b = M @ ((4.0 * u - up) / 3.0) if scheme == BDF2 else M @ u
        b -= lift @ g
        b[bc_dofs] = g
        up, u = u, lu.solve(b)
        out.append(u.copy())
    return np.array(out)


def steady_system(K, dofs, g, F):
    """(K_hat_S, b): b = F - K[:, S] g_S on the free rows, b_S = g_S."""
    b = (np.zeros(K.shape[0]) if F is None else np.array(F, dtype=np.float64)) - K[:, dofs].tocsr() @ g
    b[dofs] = g
    return ho.eliminate_dirichlet(K, dofs), b


def nl_residual(K, dofs, g, u, F=None):
    """||D^-1 (b - K_hat_S u)||_2 / ||D^-1 b||_2 of the system valued with K."""
    Khat, b = steady_system(K, dofs, g, F)
    d = Khat.diagonal()
    return float(np.linalg.norm((b - Khat @ u) / d) / max(np.linalg.norm(b / d), 1e-300))


def picard_loop(stiffness_at, dofs, g, x0, F, picard_tol, max_sweeps):
    """The Picard steady state, K(x) = stiffness_at(x):
        x_0 = the start state
        sweep k = 1, 2, ...:  K_hat_S(x_{k-1}) x_k = F - K(x_{k-1})[:, S] g_S on the free rows, (x_k)_S = g_S   (direct solve)
                              change_k = max |x_k - x_{k-1}|;  stop when change_k <= picard_tol
    Returns {"u", "changes" (per sweep), "sweeps", "converged", "nl_resid", "K" (valued at u)}."""
    dofs = np.asarray(dofs, dtype=np.int64)
    g = np.asarray(g, dtype=np.float64)
    x = np.array(x0, dtype=np.float64)
    changes = []
    for _ in range(int(max_sweeps)):
        Khat, b = steady_system(stiffness_at(x), dofs, g, F)
        xn = spla.splu(Khat.tocsc()).solve(b)
        xn[dofs] = g
        changes.append(float(np.abs(xn - x).max()))
        x = xn
        if changes[-1] <= picard_tol:
            break
    K = stiffness_at(x)
    return {"u": x, "changes": changes, "sweeps": len(changes), "converged": changes[-1] <= picard_tol,
            "nl_resid": nl_residual(K, dofs, g, x, F), "K": K}
