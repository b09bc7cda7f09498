"""Enthalpy-form restatement of the time loop (hf_set_capacity_form) for the CPU and GPU tests of the
energy-conserving cv(T) steps.  TEST CODE: never imported by heatflow_amd.

Backward Euler only.  Per step, with e the evaluation state, omega the relaxation, tol the stop tolerance and P the sweep cap:
    e_0 = u^n
    sweep k = 1, 2, ...:
        Ta_e = Tw_e(u^n), Tb_e = Tw_e(e_{k-1})          Tw_e(u) = sum_j (rs + r_j) u_j / (4 rs), rs = r_0 + r_1 + r_2
        rho_c_e = the mean of the tag's clamped capacity table over [Ta_e, Tb_e] (the constant for a tag without one)
        kappa_e = table(T_e(e_{k-1})) with the plain-mean T_e of kappa_T_oracle, or the constant
        M_k = M(rho_c), A_k = M_k + dt K(kappa);  A_k x_k = M_k u^n + dt F - A_k[:, B] g on the free rows, (x_k)_B = g
        change_k = max |x_k - e_{k-1}|;  stop when change_k <= tol or k = P;  e_k = e_{k-1} + omega (x_k - e_{k-1})
    u^{n+1} = x_k
The loop is this file's own (loops_oracle.table_loop's closure has no u^n); the element matrices, assembly and elimination are
oracle.heat_oracle's.  The stored heat the scheme conserves:
    E(u) = sum_e vol_e H_tag(e)(Tw_e(u)),  vol_e = A_e rs / 3,  H_tag(T) = int_0^T table (clamped) dT
           (rho_c T for a constant tag, and for a constant table)
"""
import numpy as np
import scipy.sparse.linalg as spla

from kappa_T_oracle import element_kappa, table_eval
from oracle import heat_oracle as ho

__all__ = ["Enthalpy", "H", "Tw", "bump_tables", "table_mean"]


def _knots(T0, dT, values):
    v = np.asarray(values, dtype=np.float64)
    return float(T0) + float(dT) * np.arange(len(v)), v


def H(T, T0, dT, values):
    """int_0^T table(clamped) dT', elementwise - from 0 K, so that a constant table gives the rho_c T of a constant tag: the
    first value times the first knot, whole trapezoids up to the segment of T, the partial piece as length x midpoint value;
    linear continuation with the end values outside the knots."""
    x, v = _knots(T0, dT, values)
    cum = np.concatenate([[0.0], np.cumsum(0.5 * (v[1:] + v[:-1]) * float(dT))])
    T = np.asarray(T, dtype=np.float64)
    Tc = np.clip(T, x[0], x[-1])
    i = np.clip(np.searchsorted(x, Tc, side="right") - 1, 0, len(x) - 2)
    w = Tc - x[i]
    inner = v[0] * x[0] + cum[i] + w * (v[i] + 0.5 * (w / float(dT)) * (v[i + 1] - v[i]))
    return inner + np.where(T < x[0], (T - x[0]) * v[0], 0.0) + np.where(T > x[-1], (T - x[-1]) * v[-1], 0.0)


def table_mean(Ta, Tb, T0, dT, values):
    """The mean of the clamped piecewise-linear table over [min, max] of Ta and Tb, elementwise and symmetric in them: the
    table at the midpoint where both lie in one segment or in one clamped range (exact for a linear piece, no cancellation as
    Tb -> Ta); otherwise (first partial piece + whole segments + last partial piece) / (max - min), pieces as length x
    midpoint value."""
    x, v = _knots(T0, dT, values)
    dT = float(dT)
    Ta, Tb = np.broadcast_arrays(np.asarray(Ta, dtype=np.float64), np.asarray(Tb, dtype=np.float64))
    lo, hi = np.minimum(Ta, Tb), np.maximum(Ta, Tb)
    n = len(x)
    cum = np.concatenate([[0.0], np.cumsum(0.5 * (v[1:] + v[:-1]) * dT)])

    def seg(T):      # -1 below the first knot, n - 1 from the last knot on, else the segment index
        return np.where(T <= x[0], -1, np.where(T >= x[-1], n - 1, np.clip(np.searchsorted(x, T, side="right") - 1, 0, n - 2)))
    sl, sh = seg(lo), seg(hi)
    out = table_eval(lo + 0.5 * (hi - lo), T0, dT, v)              # one segment / one clamped range
    far = sl != sh
    if np.any(far):
        l, h, jl, jh = lo[far], hi[far], sl[far], sh[far]
        below, above = jl < 0, jh >= n - 1
        il, ih = np.clip(jl, 0, n - 2), np.clip(jh, 0, n - 2)
        # head: from lo to the next knot (below the table: to the first knot, at the first value)
        k0 = np.where(below, 0, il + 1)
        len0 = x[k0] - l
        head = len0 * np.where(below, v[0], table_eval(l + 0.5 * len0, T0, dT, v))
        # tail: from the last knot at or below hi to hi (above the table: from the last knot, at the last value)
        k1 = np.where(above, n - 1, ih)
        len1 = h - x[k1]
        tail = len1 * np.where(above, v[-1], table_eval(x[k1] + 0.5 * len1, T0, dT, v))
        out = np.array(out, dtype=np.float64)
        out[far] = (head + (cum[k1] - cum[k0]) + tail) / (h - l)
    return out


def Tw(u, coords, tris):
    """The r-weighted element temperature sum_j (rs + r_j) u_j / (4 rs): int u r dA / int r dA of the P1 field."""
    r = np.asarray(coords, dtype=np.float64)[:, 1][np.asarray(tris)]
    rs = r.sum(axis=1)
    return ((rs[:, None] + r) * np.asarray(u, dtype=np.float64)[np.asarray(tris)]).sum(axis=1) / (4.0 * rs)


def bump_tables(tag_to_rc, tags, T0=300.0, dT=10.0, knots=51, lo=350.0, hi=450.0, latent_K=100.0):
    """{tag: (T0, dT, rho_c + hat)}: the tests' bump - a hat of base lo..hi carrying the latent heat rho_c * latent_K."""
    T = T0 + dT * np.arange(knots)
    hat = np.maximum(0.0, 1.0 - np.abs(T - 0.5 * (lo + hi)) / (0.5 * (hi - lo)))
    out = {}
    for t in tags:
        rc = float(tag_to_rc[int(t)])
        area = np.sum(0.5 * (hat[1:] + hat[:-1]) * dT)
        out[int(t)] = (T0, dT, rc + hat * (rc * latent_K / area))
    return out


class Enthalpy:
    """The scheme on one mesh: operators, loop, stored heat and balance."""

    def __init__(self, coords, tris, tags, tag_to_k, tag_to_rc, dt, bc_dofs, rhoc_tables, kappa_tables=None):
        self.coords = np.asarray(coords, dtype=np.float64)
        self.tris = np.asarray(tris, dtype=np.int64)
        self.tags = np.asarray(tags)
        self.tag_to_k, self.tag_to_rc = dict(tag_to_k), dict(tag_to_rc)
        self.dt = float(dt)
        self.dofs = np.asarray(bc_dofs, dtype=np.int64)
        self.ct, self.kt = dict(rhoc_tables or {}), dict(kappa_tables or {})
        self.n = len(self.coords)
        p = self.coords[self.tris]
        z, r = p[:, :, 0], p[:, :, 1]
        d = (z[:, 1] - z[:, 0]) * (r[:, 2] - r[:, 0]) - (z[:, 2] - z[:, 0]) * (r[:, 1] - r[:, 0])
        self.vol = 0.5 * np.abs(d) * r.sum(axis=1) / 3.0
        self.free = np.ones(self.n, dtype=bool)
        self.free[self.dofs] = False

    def chord_capacity(self, un, e):
        """rho_c_e of every element: the table's mean between Tw_e(un) and Tw_e(e), or the constant."""
        rc = np.array([float(self.tag_to_rc[int(t)]) for t in self.tags])
        Ta, Tb = Tw(un, self.coords, self.tris), Tw(e, self.coords, self.tris)
        for tag, (T0, dT, vals) in self.ct.items():
            sel = self.tags == int(tag)
            rc[sel] = table_mean(Ta[sel], Tb[sel], T0, dT, vals)
        return rc

    def element_terms(self, un, e):
        rc = self.chord_capacity(un, e)
        kappa = element_kappa(e, self.tris, self.tags, self.tag_to_k, self.kt)
        return ho.element_matrices(self.coords, self.tris, rc, kappa)

    def operators(self, un, e):
        """(M, A) = (M(chord capacity), M + dt K(kappa(e))), not eliminated."""
        Me, Ke = self.element_terms(un, e)
        return ho.assemble_csr(self.n, self.tris, Me), ho.assemble_csr(self.n, self.tris, Me + self.dt * Ke)

    def stiffness(self, e):
        _, Ke = ho.element_matrices(self.coords, self.tris, np.zeros(len(self.tris)),
                                    element_kappa(e, self.tris, self.tags, self.tag_to_k, self.kt))
        return ho.assemble_csr(self.n, self.tris, Ke)

    def enthalpy_fields(self, u0, g_all, sweeps=8, tol=0.0, relax=1.0, F=None):
        """Every step's field (n_steps x n), the sweeps used and the last change_k of every step."""
        u = np.array(u0, dtype=np.float64)
        fields, used, changes = [], [], []
        for g in np.asarray(g_all, dtype=np.float64):
            e = u.copy()
            for k in range(1, int(sweeps) + 1):
                M, A = self.operators(u, e)
                b = M @ u if F is None else M @ u + self.dt * np.asarray(F, dtype=np.float64)
                if len(self.dofs):
                    b -= A[:, self.dofs].tocsr() @ g
                    b[self.dofs] = g
                    A = ho.eliminate_dirichlet(A, self.dofs)
                x = spla.splu(A.tocsc()).solve(b)
                change = float(np.abs(x - e).max())
                if (tol > 0.0 and change <= tol) or k == int(sweeps):      # (tol = 0: every sweep runs)
                    break
                e = e + relax * (x - e)
            u = x
            fields.append(u.copy())
            used.append(k)
            changes.append(change)
        return np.array(fields), np.array(used), np.array(changes)

    def stored_heat_terms(self, u):
        """vol_e H_tag(e)(Tw_e(u)) of every element."""
        T = Tw(u, self.coords, self.tris)
        h = np.array([float(self.tag_to_rc[int(t)]) for t in self.tags]) * T
        for tag, (T0, dT, vals) in self.ct.items():
            sel = self.tags == int(tag)
            h[sel] = H(T[sel], T0, dT, vals)
        return self.vol * h

    def stored_heat(self, u):
        """{tag: sum_e vol_e H_tag(Tw_e(u))}."""
        terms = self.stored_heat_terms(u)
        return {int(t): float(terms[self.tags == t].sum()) for t in np.unique(self.tags)}

    def balance(self, u_prev, u_new, g, F=None):
        """(dE, rhs) of one step: dE = E(u_new) - E(u_prev), formed without cancellation as sum_e vol_e mean(Ta, Tb) (Tb - Ta),
        and rhs = dt sum_free (F - K(kappa(u_new)) u_new)_i + sum_B [M (u_new - u_prev)]_i with M the chord mass matrix between
        the two states.  Equal for a converged step."""
        Ta, Tb = Tw(u_prev, self.coords, self.tris), Tw(u_new, self.coords, self.tris)
        dE = float((self.vol * self.chord_capacity(u_prev, u_new) * (Tb - Ta)).sum())
        Me, _ = self.element_terms(u_prev, u_new)
        M = ho.assemble_csr(self.n, self.tris, Me)
        flux = -(self.stiffness(u_new) @ u_new)
        if F is not None:
            flux = flux + np.asarray(F, dtype=np.float64)
        rhs = self.dt * float(flux[self.free].sum()) + float((M @ (u_new - u_prev))[self.dofs].sum())
        return dE, rhs
