"""Variable time steps: the coefficient formulas, the predictor of the local-error estimate and the step
controller.  Pure Python, no backend call: the GPU path (HeatProblem.run_steps / run_adaptive) and the float64 restatement of the
tests call the same functions.

Orders: 1 = backward Euler, 2 = BDF2.  With the step sizes d0 = dt_n (the step just taken, t_n -> t_{n+1}), d1 = dt_{n-1},
d2 = dt_{n-2} and the ratio w = d0 / d1:

    BDF2 step      A' u^{n+1} = M (a u^n - b u^{n-1}) + dt' F,   A' = M + dt' K,
                   dt' = d0 (1+w)/(1+2w),   a = (1+w)^2/(1+2w),   b = w^2/(1+2w)        (w = 1: 2/3 d0, 4/3, 1/3)
    predictor      the Lagrange extrapolation of (u^n, u^{n-1}[, u^{n-2}]) to t_{n+1}: weights w0, w1[, w2]
    estimate       c (u^{n+1} - predictor),  c = d0/(d0+d1)  (order 1),  d0 (1+w)/((1+2w)(d0+d1+d2))  (order 2)

c is the local-error constant of the scheme over the error constant of the predictor (the interpolation-error residual of the
BDF-k polynomial divided by its leading coefficient); at constant step the estimates are 1/2 of the second and 2/9 of the third
backward difference.  History before the start of a run is the rest state, spaced by the first step's size.
"""
from __future__ import annotations

import math

BDF2_MAX_RATIO = 1.0 + math.sqrt(2.0)      # zero-stability limit of variable-step BDF2


def scheme_order(scheme):
    """1 for backward Euler, 2 for BDF2 (names or the library's codes)."""
    if scheme in ("backward_euler", 0):
        return 1
    if scheme in ("bdf2", 1):
        return 2
    raise ValueError(f"unknown scheme {scheme!r}")


def bdf2_coefficients(omega):
    """(a, b, f) of a BDF2 step with the ratio omega = dt_n / dt_{n-1}: the right-hand side is M (a u^n - b u^{n-1}) and the
    effective step dt' = f dt_n."""
    omega = float(omega)
    if not omega > 0.0:
        raise ValueError(f"step ratio must be positive, got {omega!r}")
    den = 1.0 + 2.0 * omega
    return (1.0 + omega) * (1.0 + omega) / den, omega * omega / den, (1.0 + omega) / den


def effective_step(order, dt, omega=1.0):
    """dt' of a step of size ``dt``: dt itself (order 1); dt (1+w)/(1+2w) (order 2), formed as the library forms it (2 dt / 3 at
    w = 1, so that a run of equal steps keeps the assembled operator bit for bit)."""
    if order == 1:
        return float(dt)
    if omega == 1.0:
        return 2.0 * dt / 3.0
    return dt * (1.0 + omega) / (1.0 + 2.0 * omega)


def predictor_weights(order, d0, d1, d2=None):
    """Weights of (u^n, u^{n-1}[, u^{n-2}]) in the extrapolation to t_{n+1} = t_n + d0."""
    if order == 1:
        return (d0 + d1) / d1, -d0 / d1
    s = d0 + d1 + d2
    return (d0 + d1) * s / (d1 * (d1 + d2)), -(d0 * s) / (d1 * d2), d0 * (d0 + d1) / ((d1 + d2) * d2)


def estimator_constant(order, d0, d1, d2=None):
    """c of the estimate c (u^{n+1} - predictor)."""
    if order == 1:
        return d0 / (d0 + d1)
    om = d0 / d1
    return d0 * (1.0 + om) / ((1.0 + 2.0 * om) * (d0 + d1 + d2))


def history_steps(steps):
    """(d0, d1, d2) for the step taken last, from the sizes of all steps since rest (oldest first): missing ones are the first
    step's size (the rest state at virtual times -dt_0, -2 dt_0)."""
    steps = list(steps)
    d0 = steps[-1]
    d1 = steps[-2] if len(steps) >= 2 else steps[0]
    d2 = steps[-3] if len(steps) >= 3 else steps[0]
    return d0, d1, d2


class StepController:
    """The textbook controller: after a step of size dt with the estimate ``err`` (same unit as ``tol``),

        factor = safety (tol / err)^(1 / (order + 1)), limited to [shrink, grow];

    the step is accepted when err <= tol; an accepted step keeps dt when the factor lies in ``keep`` (no re-valuation for a small
    gain), and the step that follows a rejection does not grow.  The band starts at 1: a step the controller would shrink is
    shrunk.  (With a band from 0.9 the steps of a rising drive stay at estimates of 0.8 .. 1.0 tol, where the next small rise of
    the estimate is a rejection: 31 of 147 solves in the smooth-pulse run of DESIGN.md 3.25, against 25 of 142.)  ``grow`` is
    capped at 2 for order 2, well inside variable-step BDF2's limit 1 + sqrt 2.  The new size is limited to [dt_min, dt_max]."""

    def __init__(self, tol, order, safety=0.9, shrink=0.25, grow=2.0, keep=(1.0, 1.2), dt_min=None, dt_max=None):
        if not (tol > 0.0 and math.isfinite(tol)):
            raise ValueError(f"tol must be positive and finite, got {tol!r}")
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, got {order!r}")
        if not (0.0 < safety <= 1.0 and 0.0 < shrink < 1.0 <= grow and keep[0] <= 1.0 <= keep[1]):
            raise ValueError("need 0 < safety <= 1, 0 < shrink < 1 <= grow and keep[0] <= 1 <= keep[1]")
        self.tol, self.order, self.safety, self.shrink = float(tol), int(order), float(safety), float(shrink)
        self.grow = min(float(grow), 2.0) if order == 2 else float(grow)
        self.keep = (float(keep[0]), float(keep[1]))
        self.dt_min = None if dt_min is None else float(dt_min)
        self.dt_max = None if dt_max is None else float(dt_max)
        self._rejected = False       # the last decision was a rejection: the step that follows it does not grow
        if self.dt_min is not None and self.dt_max is not None and self.dt_min > self.dt_max:
            raise ValueError("dt_min exceeds dt_max")

    def factor(self, err):
        if not math.isfinite(err):         # a diverged step (the library reports +inf; NaN is treated alike)
            return self.shrink
        if not err > 0.0:
            return self.grow
        return min(self.grow, max(self.shrink, self.safety * (self.tol / err) ** (1.0 / (self.order + 1))))

    def limit(self, dt):
        if self.dt_max is not None:
            dt = min(dt, self.dt_max)
        if self.dt_min is not None:
            dt = max(dt, self.dt_min)
        return dt

    def decide(self, err, dt):
        """(accepted, size of the next attempt)."""
        f = self.factor(err)
        accepted = err <= self.tol
        if accepted and self._rejected:
            f = min(f, 1.0)                # the step right after a rejection does not grow (it would be rejected again)
        self._rejected = not accepted
        if accepted and self.keep[0] <= f <= self.keep[1]:
            return True, dt
        if not accepted:
            f = min(f, self.safety)        # a rejected step never keeps or grows
        return accepted, self.limit(dt * f)

    def at_floor(self, dt):
        """The step cannot shrink further: a rejection here is a failure."""
        return self.dt_min is not None and dt <= self.dt_min

    @staticmethod
    def toward(t, dt, t_final):
        """(size, lands): the size of the step from t that does not pass t_final - the rest when dt reaches it (lands = True), half
        the rest when a full dt would leave a sliver of less than dt behind."""
        rest = t_final - t
        if dt >= rest * (1.0 - 1e-12):
            return rest, True
        if rest < 2.0 * dt:
            return 0.5 * rest, False
        return dt, False


# ---- the configuration keys timing.steps and timing.adaptive ----------------------------------------------------------------------
STEPS_KEY, ADAPTIVE_KEY = "timing.steps", "timing.adaptive"
ADAPTIVE_OPTIONS = ("tol", "dt_init", "dt_min", "dt_max", "atol", "rtol")


def timing_plan(cfg):
    """What the ``timing`` block asks of the time loop: ("uniform", num_steps), ("steps", the step sizes) for

        steps: [{until: 2.0e-6, num_steps: 80}, {until: 3.0e-5, num_steps: 40}]     # piecewise uniform, the last until = t_final

    or ("adaptive", {tol, dt_init, dt_min, dt_max, atol, rtol}) for ``adaptive: {tol: 0.1, ...}``.  ValueError naming the key for
    both keys at once, a segment list that does not rise to ``t_final``, counts below 1, an unknown option, a tolerance or step
    that is not positive.  ``num_steps`` stays required without the two keys; next to one it is ignored with a warning."""
    import warnings

    timing = cfg.get("timing") or {}
    steps, adaptive = timing.get("steps"), timing.get("adaptive")
    if steps is not None and adaptive is not None:
        raise ValueError(f"{STEPS_KEY} together with {ADAPTIVE_KEY} is not supported (one of the two)")
    if steps is None and adaptive is None:
        if timing.get("num_steps") is None:
            raise ValueError(f"timing.num_steps is required (without {STEPS_KEY} or {ADAPTIVE_KEY})")
        return "uniform", int(timing["num_steps"])
    key = STEPS_KEY if steps is not None else ADAPTIVE_KEY
    if timing.get("num_steps") is not None:
        warnings.warn(f"timing.num_steps is ignored next to {key}", RuntimeWarning, stacklevel=2)
    t_final = float(timing["t_final"])
    if steps is not None:
        if not isinstance(steps, (list, tuple)) or not steps:
            raise ValueError(f"{STEPS_KEY}: a non-empty list of {{until, num_steps}} expected")
        dts, t = [], 0.0
        for k, seg in enumerate(steps):
            if not isinstance(seg, dict) or set(seg) != {"until", "num_steps"}:
                raise ValueError(f"{STEPS_KEY}[{k}]: the keys until and num_steps expected, got {seg!r}")
            until, n = float(seg["until"]), int(seg["num_steps"])
            if n < 1 or int(seg["num_steps"]) != seg["num_steps"]:
                raise ValueError(f"{STEPS_KEY}[{k}]: num_steps must be a whole number >= 1, got {seg['num_steps']!r}")
            if not (math.isfinite(until) and until > t):
                raise ValueError(f"{STEPS_KEY}[{k}]: until = {until!r} does not lie beyond the segment before it ({t!r})")
            dts += [(until - t) / n] * n
            t = until
        if t != t_final:
            raise ValueError(f"{STEPS_KEY}: the last until ({t!r}) must equal timing.t_final ({t_final!r})")
        return "steps", dts
    if not isinstance(adaptive, dict) or "tol" not in adaptive:
        raise ValueError(f"{ADAPTIVE_KEY}: a mapping with tol expected, got {adaptive!r}")
    unknown = sorted(set(adaptive) - set(ADAPTIVE_OPTIONS))
    if unknown:
        raise ValueError(f"{ADAPTIVE_KEY}: unknown key {unknown[0]!r} ({', '.join(ADAPTIVE_OPTIONS)})")
    opts = {}
    for name in ADAPTIVE_OPTIONS:
        v = adaptive.get(name)
        if v is None:
            continue
        v = float(v)
        if not (math.isfinite(v) and (v > 0.0 or (name == "rtol" and v == 0.0))):
            raise ValueError(f"{ADAPTIVE_KEY}.{name} must be positive and finite, got {adaptive[name]!r}")
        opts[name] = v
    return "adaptive", opts


def assembled_step(cfg):
    """The step the operator is assembled with (and the multigrid hierarchy built for): t_final / num_steps; under
    ``timing.steps`` the first step; under ``timing.adaptive`` dt_init, or t_final / 400."""
    kind, data = timing_plan(cfg)
    t_final = float(cfg["timing"]["t_final"])
    if kind == "uniform":
        return t_final / data
    if kind == "steps":
        return data[0]
    return data.get("dt_init", t_final / 400.0)


def refuse_variable_steps(cfg, where):
    """ValueError naming both keys if ``cfg`` carries ``timing.steps`` or ``timing.adaptive``: ``where`` - the sweeps, run_batch,
    tangents=, monitor_sigma=, heatflow_amd.fit, the enthalpy form, the read-flux run, the 1-D model - steps with
    t_final / num_steps only."""
    timing = cfg.get("timing") or {}
    for key, name in ((STEPS_KEY, "steps"), (ADAPTIVE_KEY, "adaptive")):
        if timing.get(name) is not None:
            raise ValueError(f"{where} together with {key} is not supported ({STEPS_KEY} / {ADAPTIVE_KEY} cover the single forward "
                             "run; this path takes equal steps of t_final / num_steps)")
