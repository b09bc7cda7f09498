"""Exact reference of the table evaluators (ktab_eval, ktab_mean of hf_kernels.hpp; the stored-heat term of k_stored_heat) in
rational arithmetic, a branch classifier, and the rounding model the device is held to.  TEST CODE: never imported by heatflow_amd.

Exact side.  Every float64 input is the rational it is (fractions.Fraction; inside, integers on one power-of-two scale, since
every float64 is a dyadic rational).  The knots sit at t0 + i dT exactly - not at the float64 nearest to it - and s = (T - t0) / dT.
    value(T)          the clamped piecewise-linear table
    integral(Ta, Tb)  int_Ta^Tb of it (signed), from the antiderivative H(T) = int_t0^T: (T - t0) v_0 below the table,
                      P_i + w v_i + w^2 (v_{i+1} - v_i) / (2 dT) in segment i (w = T - knot i, P_i the whole trapezoids before it),
                      P_{n-1} + (T - knot n-1) v_{n-1} above it
    mean(Ta, Tb)      integral / (Tb - Ta), value(Ta) where Ta == Tb
    heat_term(vol, T_ref, Tw) = vol * mean(T_ref, Tw) * (Tw - T_ref) = vol * integral(T_ref, Tw)
    classify_point / classify_pair: which case of ktab_eval / ktab_mean an argument belongs to, from exact s

Element temperatures are inputs of the evaluators, not part of them: element_T and element_Tw restate their documented bits in
float64 numpy (sorted_sum3 = (lo + mid) + hi of three values sorted by value; T_e = sorted_sum3(u) * (1.0 / 3.0);
Tw_e = sorted_sum3((rs + r_j) u_j) / (4 rs), rs = sorted_sum3(r)), and those floats go into the exact functions.

Rounding model (derived, not measured).  u = 2^-53.  Every rounding of the device statements is charged one full ulp of its
result, |fl(x) - x| <= 2^-52 |x| = 2 u |x|, which holds whichever way the last bit is rounded.  This factor 2 over
round-to-nearest is a margin and not a term: where one rounding dominates (the final sum of ktab_eval on a table whose slope is
small against its value) a float64 evaluation attains that rounding's bound almost fully - measured 0.42 of a count at u per
rounding - and no worst-case first-order count can lie four times above what it bounds there.  The margin is what keeps the
replicas of tests/test_table_exact_cpu.py under 1/4 of the model (0.21); nothing else in the model is scaled.
V = the largest |v_i| over the knots an evaluation reads, D = the largest |v_{i+1} - v_i| over the segments it can read: the segments of the exact arguments and the neighbour a
rounded s can fall into (the table is continuous, so an evaluation in the neighbouring segment at the rounded s is the table at
the rounded s; outside the table the slope is 0).

ktab_eval:  s^ = fl(fl(T - t0) * fl(1 / dT)) carries three roundings, |s^ - s| <= 3 (2u) |s|; an input that lies one ulp from the
device's (a replica of T_e / Tw_e one ulp off) moves s by 2u |T| / dT more (ulp(T) <= 2^-52 |T|):
    ds(T) = 2u (3 |s| + |T| / dT).
i = int(s^) and s^ - i are exact (Sterbenz for i >= 1).  b - a, the product with the fraction f <= 1 and the sum are one
rounding each: 2u (|v| + 2 f |b - a|).  With the slope |b - a| per knot on ds:
    model_eval = 2u (|v| + |b - a| (2 + 3 |s| + |T| / dT))  <=  2u (V + D (2 + 3 |s| + |T| / dT)).

ktab_mean.  The mean is continuous in both ends with |d mean / d s_end| = |v(s_end) - mean| / (sh - sl) <= D, so the rounded
ends cost D (ds(Ta) + ds(Tb)) whichever branch the device takes, and the device's branch at the rounded ends is bounded with
that branch's own statements:
  one segment / one clamped range: sm = fl(sl + fl(0.5 fl(sh - sl))) is two roundings of at most max |s| (D 2 (2u) max |s|),
      then ktab_eval's three: 2u (V + 2 D).
  otherwise, with w = sh - sl, L_h and L_t the lengths of the head and tail pieces (L_h + N + L_t = w, N the whole segments
  between) and C the largest |cum| read:
      head = fl(L (a + g (b - a))): 1 - x, x + 1, b - a, the product, the sum and the outer product: <= 3 (2u) L_h (V + D)
      tail: fewer roundings of the same shapes:                                                   <= 3 (2u) L_t (V + D)
      cum[k] = fl(cum[k-1] + fl(0.5 fl(v_{k-1} + v_k))) (kt_ensure_cum): the roundings before knot jl are common to cum[ih] and
      cum[jl] and cancel in the difference; each of the N steps between adds at most 2u (|cum_k| + |trapezoid_k|) <= 2 (2u) C, and
      the subtraction one more rounding of |diff| <= C:                                          <= (2u) (2 N + 1) C, 0 for N = 0
      (cum[k] - cum[k] is exactly 0: a pair straddling one knot pays nothing here, however narrow it is)
      the two sums: 2 (2u) (|head| + |diff| + |tail|) <= 2 (2u) V w;  sh - sl and the division: 2 (2u) |mean| <= 2 (2u) V
  divided by w, with (L_h + L_t) / w <= 1:  2u (7 V + 3 D + (2 N + 1) C / w).
  A rounded end on the other side of a knot gives the device one whole segment more or fewer than the exact ends have; N counts
  one more whenever w + 2 (ds(Ta) + ds(Tb)) >= 1, i.e. whenever the rounded ends can be a whole segment apart (ends a rounding
  inside two neighbouring knots make the device form cum[k] - cum[k-1] at w just under 1).  Below that at most one knot lies
  between the rounded ends and both counts are 0.
    model_mean = 2u (7 V + 3 D + [w + 2 ds >= 1] (2 (N + 1) + 1) C / w) + D (ds(Ta) + ds(Tb) + 4u max |s|).
Both clamped ranges return a table value exactly: a pair wholly inside one of them, rounded ends included, has the model 0 (and
so has ktab_eval wherever D = 0: a + f * 0 is a).

Matrix entries (tests/test_gpu_table_edges.py): an entry of M is bounded by sum over its triangles |M_e,ij| model_e / c_e plus
1e-13 of the entry's summands for the float64 geometry (the project's figure for matrix entries); the stored heat per
tag by the same sum over |term_e|; an entry of A on |M_ij| + dt |K_ij| (test_gpu_rhoc_T.py's convention).
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
_S = 400                                   # every input is an integer multiple of 2^-_S (|x| >= 2^-347 or 0)
_ONE = 1 << _S

POINT_CLASSES = ("below", "above", "segment", "knot")


def scaled(x):
    """The float64 x as an integer multiple of 2^-_S."""
    n, d = float(x).as_integer_ratio()
    q, r = divmod(_ONE, d)
    if r:
        raise ValueError(f"{x!r} is finer than 2^-{_S}")
    return n * q


def sorted_sum3(a, b, c):
    """(lo + mid) + hi of three values sorted by value, elementwise (hf_kernels.hpp's sorted_sum3)."""
    a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
    ab_lo, ab_hi = np.minimum(a, b), np.maximum(a, b)
    lo, hi, mid = np.minimum(ab_lo, c), np.maximum(ab_hi, c), np.maximum(ab_lo, np.minimum(ab_hi, c))
    return (lo + mid) + hi


def element_T(u, tris):
    """T_e = sorted_sum3(u) * (1.0 / 3.0): the plain-mean element temperature (element_temperature)."""
    v = np.asarray(u, dtype=np.float64)[np.asarray(tris)]
    return sorted_sum3(v[:, 0], v[:, 1], v[:, 2]) * (1.0 / 3.0)


def element_Tw(u, coords, tris):
    """Tw_e = sorted_sum3((rs + r_j) u_j) / (4 rs), rs = sorted_sum3(r): the r-weighted element temperature (element_tw)."""
    tris = np.asarray(tris)
    r = np.asarray(coords, dtype=np.float64)[:, 1][tris]
    v = np.asarray(u, dtype=np.float64)[tris]
    rs = sorted_sum3(r[:, 0], r[:, 1], r[:, 2])
    return sorted_sum3((rs + r[:, 0]) * v[:, 0], (rs + r[:, 1]) * v[:, 1], (rs + r[:, 2]) * v[:, 2]) / (4.0 * rs)


def element_volume(coords, tris):
    """vol_e = ((0.5 |d|) * ((r0 + r1) + r2)) / 3.0 as k_stored_heat forms it."""
    p = np.asarray(coords, dtype=np.float64)[np.asarray(tris)]
    z, r = p[:, :, 0], p[:, :, 1]
    d = (z[:, 1] - z[:, 0]) * (r[:, 2] - r[:, 0]) - (z[:, 2] - z[:, 0]) * (r[:, 1] - r[:, 0])
    return ((0.5 * np.abs(d)) * ((r[:, 0] + r[:, 1]) + r[:, 2])) / 3.0


def pair_classes(tab):
    """The classes of classify_pair that a table can meet.  A straddled knot needs an inner knot, two need two; a variant with an
    end exactly on a knot needs a knot that is a float64 where that end can lie (the first knot, t0, always is one)."""
    n, fk = tab.n, tab.float_knots()
    out = ["below", "above", "one_segment", "below_into_interior", "interior_into_above", "below_through_above",
           "equal:below", "equal:above", "equal:segment", "equal:knot",
           "one_segment+knot", "below+knot", "interior_into_above+knot"]              # knot 0 serves these three
    if n - 1 in fk:
        out.append("above+knot")
    if any(k >= 1 for k in fk):
        out.append("below_into_interior+knot")
    if n >= 3:
        out.append("straddle_one_knot")
        if any(k <= n - 3 or k >= 2 for k in fk):
            out.append("straddle_one_knot+knot")
    if n >= 4:
        out.append("span_knots")
        if any(k <= n - 4 or k >= 3 for k in fk):
            out.append("span_knots+knot")
    return out


class ExactTable:
    """One table (T0, dT, values) in exact arithmetic."""

    def __init__(self, T0, dT, values):
        self.T0, self.dT = float(T0), float(dT)
        self.v = np.asarray(values, dtype=np.float64).ravel()
        self.n = len(self.v)
        if self.n < 2 or not self.dT > 0.0:
            raise ValueError("a table needs two knots and dT > 0")
        self.x0, self.dt = scaled(self.T0), scaled(self.dT)
        self.vi = [scaled(x) for x in self.v]
        self.top = (self.n - 1) * self.dt
        self.p2 = [0]                              # 2 * whole trapezoids before knot i, on the scale 2^-2S
        for j in range(self.n - 1):
            self.p2.append(self.p2[-1] + (self.vi[j] + self.vi[j + 1]) * self.dt)
        # float64 side of the model: the host's cum recurrence (knot units) and |differences| padded with the clamps' 0
        self.cum = np.zeros(self.n)
        for i in range(1, self.n):
            self.cum[i] = self.cum[i - 1] + 0.5 * (self.v[i - 1] + self.v[i])
        self.absdv = np.concatenate([[0.0], np.abs(np.diff(self.v)), [0.0]])      # index j + 1: segment j; 0 and n: the clamps

    # ---- exact ------------------------------------------------------------------------------------------------------------------
    def _locate(self, t):
        d = t - self.x0
        if d <= 0:
            return -1, 0, d
        if d >= self.top:
            return 1, self.n - 1, d - self.top
        i, w = divmod(d, self.dt)
        return 0, i, w

    def s(self, T):
        return Fraction(scaled(T) - self.x0, self.dt)

    def knot(self, i):
        """Knot i as a Fraction (t0 + i dT exactly; in general no float64)."""
        return Fraction(self.x0 + i * self.dt, _ONE)

    def float_knots(self):
        """The knots that are float64 numbers: the only ones an argument can lie on exactly."""
        return [k for k in range(self.n) if Fraction(float(self.knot(k))) == self.knot(k)]

    def value(self, T):
        reg, i, w = self._locate(scaled(T))
        if reg:
            return Fraction(self.vi[0 if reg < 0 else -1], _ONE)
        return Fraction(self.vi[i] * self.dt + w * (self.vi[i + 1] - self.vi[i]), self.dt * _ONE)

    def _h2(self, t):
        """2 dT * int_t0^t of the clamped table, on the scale 2^-3S."""
        reg, i, w = self._locate(t)
        if reg < 0:
            return 2 * self.dt * w * self.vi[0]
        if reg > 0:
            return self.dt * (self.p2[-1] + 2 * w * self.vi[-1])
        return self.dt * (self.p2[i] + 2 * w * self.vi[i]) + w * w * (self.vi[i + 1] - self.vi[i])

    def integral(self, Ta, Tb):
        return Fraction(self._h2(scaled(Tb)) - self._h2(scaled(Ta)), 2 * self.dt * _ONE * _ONE)

    def mean(self, Ta, Tb):
        a, b = scaled(Ta), scaled(Tb)
        if a == b:
            return self.value(Ta)
        return Fraction(self._h2(b) - self._h2(a), 2 * self.dt * (b - a) * _ONE)

    def heat_term(self, vol, T_ref, Tw):
        """vol * mean(T_ref, Tw) * (Tw - T_ref)."""
        return Fraction(float(vol)) * self.integral(T_ref, Tw)

    # ---- classes ----------------------------------------------------------------------------------------------------------------
    def classify_point(self, T):
        d = scaled(T) - self.x0
        if d < 0:
            return "below"
        if d > self.top:
            return "above"
        return "knot" if d % self.dt == 0 else "segment"

    def classify_pair(self, Ta, Tb):
        a, b = scaled(Ta) - self.x0, scaled(Tb) - self.x0
        if a == b:
            return "equal:" + self.classify_point(Ta)
        if a > b:
            a, b = b, a
        top, dt = self.top, self.dt
        if b <= 0:
            return "below" + ("+knot" if b == 0 else "")
        if a >= top:
            return "above" + ("+knot" if a == top else "")
        if a < 0 and b > top:
            return "below_through_above"
        if a < 0:
            return "below_into_interior" + ("+knot" if b % dt == 0 else "")
        if b > top:
            return "interior_into_above" + ("+knot" if a % dt == 0 else "")
        inside = -((-b) // dt) - 1 - a // dt                     # knots strictly between the ends
        base = "one_segment" if inside == 0 else "straddle_one_knot" if inside == 1 else "span_knots"
        return base + ("+knot" if a % dt == 0 or b % dt == 0 else "")

    # ---- the model (float64 arithmetic on the bound itself) ---------------------------------------------------------------------
    def _s_ds(self, T):
        T = np.asarray(T, dtype=np.float64)
        s = (T - self.T0) / self.dT
        return s, 2.0 * U * (3.0 * np.abs(s) + np.abs(T) / self.dT)

    def _reach(self, s_lo, s_hi):
        """(V, D, first knot, last knot) over the segments and knots an evaluation between s_lo and s_hi can read."""
        n = self.n
        j0 = np.clip(np.floor(s_lo), -1, n - 1).astype(np.int64)                  # -1 / n - 1: the clamps
        j1 = np.clip(np.floor(s_hi), -1, n - 1).astype(np.int64)
        k0, k1 = np.clip(j0, 0, n - 1), np.clip(j1 + 1, 0, n - 1)
        V, D = np.zeros(len(j0)), np.zeros(len(j0))
        absv = np.abs(self.v)
        for q in range(len(j0)):                                                     # (short ranges except for the widest pairs)
            V[q] = absv[k0[q]:k1[q] + 1].max()
            D[q] = self.absdv[j0[q] + 1:j1[q] + 2].max()
        return V, D, k0, k1

    def model_eval(self, T):
        """The bound on |ktab_eval - value| at every T."""
        s, ds = self._s_ds(np.atleast_1d(T))
        V, D, _, _ = self._reach(s - 2.0 * ds, s + 2.0 * ds)
        inside = D > 0.0
        return np.where(inside, 2.0 * U * (V + 2.0 * D) + D * ds, 0.0)

    def model_mean(self, Ta, Tb):
        """The bound on |ktab_mean - mean| at every pair."""
        Ta, Tb = np.atleast_1d(np.asarray(Ta, dtype=np.float64)), np.atleast_1d(np.asarray(Tb, dtype=np.float64))
        lo, hi = np.minimum(Ta, Tb), np.maximum(Ta, Tb)
        sl, dsl = self._s_ds(lo)
        sh, dsh = self._s_ds(hi)
        V, D, k0, k1 = self._reach(sl - 2.0 * dsl, sh + 2.0 * dsh)
        w = sh - sl
        n = self.n
        jl = np.where(sl > 0.0, np.clip(np.floor(sl), 0, n - 2) + 1, 0).astype(np.int64)
        ih = np.where(sh >= n - 1, n - 1, np.clip(np.floor(sh), 0, n - 2)).astype(np.int64)
        N = np.maximum(ih - jl, 0)
        C = np.array([np.abs(self.cum[a:b + 1]).max() for a, b in zip(k0, k1)])
        wide = w + 2.0 * (dsl + dsh) >= 1.0                                        # a rounded end may add a whole segment
        cum_term = np.where(wide, (2.0 * (N + 1) + 1.0) * C / np.where(wide, w, 1.0), 0.0)
        smax = np.maximum(np.abs(sl), np.abs(sh))
        reach = (D > 0.0) | ((sh + 2.0 * dsh > 0.0) & (sl - 2.0 * dsl < n - 1.0))      # not wholly inside one clamped range
        return np.where(reach, 2.0 * U * (7.0 * V + 3.0 * D + cum_term) + D * (dsl + dsh + 4.0 * U * smax), 0.0)


def abs_err(got, exact):
    """|got - exact| as a float, got a float64 and exact a Fraction."""
    return float(abs(Fraction(float(got)) - exact))
