"""Variable time steps without a GPU: the coefficient formulas, the order of variable-step BDF2, the step
controller, HeatProblem.run_steps / run_adaptive on the float64 restatement of tests/varstep_oracle.py, and the conditions the
GPU's adaptive run is held to, checked on the restatement first."""
import math

import numpy as np
import pytest

from varstep_oracle import VarstepOracleBackend, oside_node, small, smooth_problem, smooth_references, step_list

from heatflow_amd import hip_backend, stepping
from heatflow_amd.stepping import StepController


def test_formulas_at_constant_step():
    a, b, f = stepping.bdf2_coefficients(1.0)
    assert (a, b, f) == (4.0 / 3.0, 1.0 / 3.0, 2.0 / 3.0)
    assert stepping.effective_step(1, 0.3) == 0.3 and stepping.effective_step(2, 0.3) == 2.0 * 0.3 / 3.0
    assert stepping.predictor_weights(1, 0.3, 0.3) == (2.0, -1.0)
    assert stepping.estimator_constant(1, 0.3, 0.3) == 0.5
    assert np.allclose(stepping.predictor_weights(2, 0.3, 0.3, 0.3), (3.0, -3.0, 1.0), rtol=1e-15)
    assert stepping.estimator_constant(2, 0.3, 0.3, 0.3) == pytest.approx(2.0 / 9.0, rel=1e-15)
    assert stepping.BDF2_MAX_RATIO == 1.0 + math.sqrt(2.0)
    assert stepping.history_steps([0.1]) == (0.1, 0.1, 0.1) and stepping.history_steps([0.1, 0.2]) == (0.2, 0.1, 0.1)
    assert stepping.history_steps([0.1, 0.2, 0.3, 0.4]) == (0.4, 0.3, 0.2)


@pytest.mark.parametrize("omega", [0.25, 0.7, 1.0, 1.9, 2.4])
def test_formulas_are_exact_on_polynomials(omega):
    """The BDF2 step differentiates quadratics exactly, and the predictors reproduce polynomials of their degree, on any grid."""
    d0, d1, d2 = omega * 0.2, 0.2, 0.13
    a, b, f = stepping.bdf2_coefficients(omega)
    for q in (lambda t: 1.0 + 0.0 * t, lambda t: 2.0 - 3.0 * t, lambda t: 0.5 + t - 4.0 * t * t):
        t1 = 1.0 + d0
        dq = (q(t1 + 1e-6) - q(t1 - 1e-6)) / 2e-6
        assert q(t1) - a * q(1.0) + b * q(1.0 - d1) == pytest.approx(f * d0 * dq, abs=1e-9)     # u^{n+1} - a u^n + b u^{n-1} = dt' u'
        w = stepping.predictor_weights(2, d0, d1, d2)
        assert w[0] * q(1.0) + w[1] * q(1.0 - d1) + w[2] * q(1.0 - d1 - d2) == pytest.approx(q(t1), abs=1e-12)
    w = stepping.predictor_weights(1, d0, d1)
    assert w[0] * 5.0 + w[1] * (5.0 - 2.0 * d1) == pytest.approx(5.0 + 2.0 * d0, abs=1e-12)
    # the estimate of a cubic (quadratic) is c * the predictor's error = the scheme's local error constant times u''' (u'')
    cubic = lambda t: t ** 3
    w = stepping.predictor_weights(2, d0, d1, d2)
    pred_err = cubic(d0) - (w[0] * cubic(0.0) + w[1] * cubic(-d1) + w[2] * cubic(-d1 - d2))
    assert pred_err == pytest.approx(d0 * (d0 + d1) * (d0 + d1 + d2), rel=1e-12)
    # the true local error: u' = 3 t^2 solved by one BDF2 step from the exact history 0 (at t = 0) and -d1^3
    x = a * 0.0 - b * cubic(-d1)
    u1 = (x + f * d0 * 3.0 * d0 * d0)           # the right-hand side is known: u^{n+1} = a u^n - b u^{n-1} + dt' u'(t_{n+1})
    lte = cubic(d0) - u1
    assert abs(lte) == pytest.approx(d0 * d0 * (d0 + d1) ** 2 / (2.0 * d0 + d1), rel=1e-12)
    assert stepping.estimator_constant(2, d0, d1, d2) * pred_err == pytest.approx(abs(lte), rel=1e-12)
    # and for backward Euler: u = t^2, u^{n+1} = u^n + d0 u'(t_{n+1})
    w = stepping.predictor_weights(1, d0, d1)
    pe = d0 * d0 - (w[0] * 0.0 + w[1] * d1 * d1)
    assert stepping.estimator_constant(1, d0, d1) * pe == pytest.approx(abs(d0 * d0 - 2.0 * d0 * d0), rel=1e-12)


def _halve(d):
    return np.repeat(np.asarray(d) / 2.0, 2)


def test_variable_step_bdf2_is_second_order():
    """A list graded by 1.15 per step (24 steps over 4 us of the smooth pulse) and the same list with every step halved, again
    and again: the error at the end against the list halved five times falls by r1 = 4.99 at the first halving; the two further
    halvings give 5.34 and 4.50 (the last steps of the graded list are long: the ratios approach 4 from above).  r1 is held to the
    band those two span, half a unit wide on either side, and to the 3 that separates it from first order's 2."""
    case = small("with_diamond")
    base = 1.15 ** np.arange(24)
    lists = [base * (4.0e-6 / base.sum())]
    for _ in range(5):
        lists.append(_halve(lists[-1]))
    ends = []
    for d in lists:
        prob = smooth_problem(case, backend=VarstepOracleBackend(), scheme="bdf2")
        prob.run_steps(d, time_varying=[prob.bcs[3]], consistent_start=True)
        ends.append(prob.state())
    err = [float(np.abs(e - ends[-1]).max()) for e in ends[:-1]]
    r1, r2, r3 = err[0] / err[1], err[1] / err[2], err[2] / err[3]
    print(f"errors {err}, ratios {r1:.3f} {r2:.3f} {r3:.3f}")
    assert r1 >= 3.0
    assert min(r2, r3) - 0.5 <= r1 <= max(r2, r3) + 0.5


def test_controller_decisions():
    c = StepController(0.1, 2)
    assert c.decide(0.1 * 0.9 ** 3 / 1.1 ** 3, 1.0) == (True, 1.0)           # factor 1.1: inside the band, the step is kept
    ok, dt = c.decide(0.1 * 0.9 ** 3 / 1.5 ** 3, 1.0)
    assert ok and dt == pytest.approx(1.5)
    ok, dt = c.decide(0.1 * 0.9 ** 3 / 0.95 ** 3, 1.0)                       # accepted, but the controller wants less: shrunk
    assert ok and dt == pytest.approx(0.95)
    assert c.decide(1e-9, 1.0) == (True, 2.0) and c.decide(0.0, 1.0) == (True, 2.0)
    ok, dt = c.decide(0.2, 1.0)
    assert not ok and dt == pytest.approx(0.9 * 0.5 ** (1.0 / 3.0))
    ok, dt = c.decide(1e-9, 1.0)                                             # right after a rejection: no growth
    assert ok and dt == 1.0
    assert c.decide(1e-9, 1.0) == (True, 2.0)
    assert c.decide(1e9, 1.0) == (False, 0.25) and c.decide(float("inf"), 1.0) == (False, 0.25)
    assert c.decide(float("nan"), 1.0)[0] is False
    b = StepController(0.3, 1)
    ok, dt = b.decide(0.6, 1.0)
    assert not ok and dt == pytest.approx(0.9 * 0.5 ** 0.5)
    # the cap of the growth under BDF2, and none under backward Euler
    assert StepController(0.1, 2, grow=5.0).grow == 2.0 < stepping.BDF2_MAX_RATIO and StepController(0.1, 1, grow=5.0).grow == 5.0
    lim = StepController(0.1, 2, dt_min=0.5, dt_max=1.5)
    assert lim.decide(1e9, 1.0) == (False, 0.5) and lim.at_floor(0.5) and not lim.at_floor(0.6)
    assert lim.decide(1e-9, 1.0) == (True, 1.0) and lim.decide(1e-9, 1.0) == (True, 1.5)
    for bad in (dict(tol=0.0), dict(tol=float("nan")), dict(order=3), dict(safety=0.0), dict(shrink=1.0), dict(grow=0.5),
                dict(keep=(1.1, 1.2)), dict(dt_min=2.0, dt_max=1.0)):
        kw = dict(tol=0.1, order=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            StepController(**kw)


def test_controller_lands_on_t_final():
    assert StepController.toward(0.0, 0.3, 1.0) == (0.3, False)
    assert StepController.toward(0.7, 0.3, 1.0) == (1.0 - 0.7, True)
    assert StepController.toward(0.5, 0.3, 1.0) == (0.25, False)             # a full step would leave a sliver of 0.2
    assert StepController.toward(0.9, 5.0, 1.0) == (1.0 - 0.9, True)
    t, dt, n = 0.0, 0.037, 0
    while True:
        h, lands = StepController.toward(t, dt, 1.0)
        assert 0.0 < h <= dt * (1.0 + 1e-12)
        n += 1
        if lands:
            assert t + h == pytest.approx(1.0, abs=1e-15)
            break
        t += h
    assert n == 28


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_run_steps_on_the_restatement(scheme):
    case = small("with_diamond")
    prob = smooth_problem(case, backend=VarstepOracleBackend(), scheme=scheme)
    dts = step_list(prob.dt)
    nodes = np.arange(0, prob.n, 7, dtype=np.int32)
    times, s, iters = prob.run_steps(dts, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
    assert np.array_equal(times, np.cumsum(dts)) and s.shape == (12, len(nodes)) and len(iters) == 12
    info = prob.backend.step_info()
    assert info["t"] == times[-1] and info["dt_last"] == dts[-1] and info["revaluations"] == (9 if scheme == "backward_euler" else 10)
    # the list is cleared: the next plain run takes the assembled step again, and continues the time
    t2, _, _ = prob.run(1, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
    assert prob.backend.step_info()["dt_last"] == prob.dt
    # equal steps are the constant-step run
    one = smooth_problem(case, backend=VarstepOracleBackend(), scheme=scheme)
    two = smooth_problem(case, backend=VarstepOracleBackend(), scheme=scheme)
    _, s1, _ = one.run_steps([one.dt] * 5, watcher_nodes=nodes, time_varying=[one.bcs[3]])
    _, s2, _ = two.run(5, watcher_nodes=nodes, time_varying=[two.bcs[3]])
    assert np.array_equal(s1, s2) and one.backend.step_info()["revaluations"] == 0
    for bad in ([], [1e-8, 0.0], [1e-8, float("nan")], [-1e-8]):
        with pytest.raises(ValueError, match="run_steps"):
            one.run_steps(bad)
    if scheme == "bdf2":
        with pytest.raises(ValueError, match="sqrt 2"):
            one.run_steps([one.dt, 2.5 * one.dt], time_varying=[one.bcs[3]])


def test_adaptive_run_on_the_restatement_meets_the_conditions_of_the_gpu_test():
    """BDF2, tol 0.1 K, 30 us under the smooth pulse: at most 400 solves, the o-side error against 6400 fixed steps no larger
    than that of 800 fixed steps, the last step lands on t_final, and the replay of the accepted sizes as a list gives the same
    watcher curve bit for bit."""
    case = small("with_diamond")
    node = oside_node(case)
    (t_ref, o_ref), err800 = smooth_references()
    prob = smooth_problem(case, backend=VarstepOracleBackend(), scheme="bdf2")
    times, s, iters, info = prob.run_adaptive(3.0e-5, 0.1, watcher_nodes=node, time_varying=[prob.bcs[3]])
    err = float(np.abs(s[:, 0] - np.interp(times, t_ref, o_ref)).max())
    print(f"adaptive BDF2 tol 0.1 K on the restatement: {info['accepted']} + {info['rejected']} solves, {info['revaluations']} "
          f"re-valuations, steps {info['dt'].min():.2e} .. {info['dt'].max():.2e} s, o-side error {err:.4f} K; 800 fixed steps: {err800:.4f} K")
    assert times[-1] == 3.0e-5 and np.all(np.diff(times) > 0.0) and len(iters) == info["accepted"] == len(info["dt"])
    assert np.all(info["err"] <= 0.1) and (info["dt"][1:] / info["dt"][:-1]).max() <= 2.0 + 1e-12
    assert info["accepted"] + info["rejected"] <= 400
    assert err <= err800
    replay = smooth_problem(case, backend=VarstepOracleBackend(), scheme="bdf2")
    t2, s2, _ = replay.run_steps(info["dt"], watcher_nodes=node, time_varying=[replay.bcs[3]], consistent_start=True)
    assert np.array_equal(s2, s) and np.abs(t2 - times).max() <= 1e-18
    # afterwards the assembled step is in force again: run() steps with dt, at the times it reports
    assert prob.backend.step_info()["dt_last"] == info["dt"][-1]
    prob.run(2, watcher_nodes=node, time_varying=[prob.bcs[3]])
    assert prob.backend.step_info()["dt_last"] == prob.dt and prob.backend.step_info()["t"] == pytest.approx(3.0e-5 + 2 * prob.dt, rel=1e-14)


def test_the_keep_band_of_the_prototype_misses_the_accuracy_condition():
    """Why the controller's keep band starts at 1: with the prototype's (0.9, 1.2) the same run takes 116 + 31
    solves and ends 0.1224 K off on the o-side, above the 0.1188 K of 800 fixed steps; from 1.0 it takes 117 + 25 and 0.1178 K."""
    case = small("with_diamond")
    node = oside_node(case)
    (t_ref, o_ref), err800 = smooth_references()
    prob = smooth_problem(case, backend=VarstepOracleBackend(), scheme="bdf2")
    times, s, _, info = prob.run_adaptive(3.0e-5, 0.1, watcher_nodes=node, time_varying=[prob.bcs[3]], keep=(0.9, 1.2))
    err = float(np.abs(s[:, 0] - np.interp(times, t_ref, o_ref)).max())
    print(f"keep (0.9, 1.2): {info['accepted']} + {info['rejected']} solves, o-side error {err:.4f} K; 800 fixed steps: {err800:.4f} K")
    assert info["accepted"] + info["rejected"] <= 400
    assert err > err800 and info["rejected"] > 25


def test_adaptive_run_under_backward_euler_and_the_floor():
    case = small("with_diamond")
    node = oside_node(case)
    (t_ref, o_ref), _ = smooth_references()
    prob = smooth_problem(case, backend=VarstepOracleBackend(), scheme="backward_euler")
    times, s, _, info = prob.run_adaptive(3.0e-5, 0.3, watcher_nodes=node, time_varying=[prob.bcs[3]])
    err = float(np.abs(s[:, 0] - np.interp(times, t_ref, o_ref)).max())
    print(f"adaptive backward Euler tol 0.3 K on the restatement: {info['accepted']} + {info['rejected']} solves, o-side error {err:.3f} K")
    assert times[-1] == 3.0e-5 and info["accepted"] + info["rejected"] <= 400 and err <= 1.52     # 800 fixed steps: 1.52 K
    floor = smooth_problem(case, backend=VarstepOracleBackend(), scheme="bdf2")
    with pytest.raises(hip_backend.NotConverged, match="dt_min"):
        floor.run_adaptive(3.0e-5, 1e-4, time_varying=[floor.bcs[3]], dt_init=1e-7, dt_min=5e-8)
    floor.run(1, time_varying=[floor.bcs[3]])                 # left through the exception: the assembled step all the same
    assert floor.backend.step_info()["dt_last"] == floor.dt
    with pytest.raises(ValueError, match="consistent start"):  # a run under way cannot be given a consistent start
        floor.run_steps([floor.dt], time_varying=[floor.bcs[3]], consistent_start=True)
    with pytest.raises(ValueError, match="consistent start"):
        floor.run_adaptive(1.0, 0.1, time_varying=[floor.bcs[3]])
    with pytest.raises(ValueError, match="t_final"):
        floor.run_adaptive(0.0, 0.1)
    with pytest.raises(ValueError, match="callable"):
        floor.run_adaptive(1e-6, 0.1, source_amplitude=[1.0])


def test_rejection_on_the_restatement_restores_the_step_before():
    case = small("with_diamond")
    prob = smooth_problem(case, backend=VarstepOracleBackend(), scheme="bdf2")
    be = prob.backend
    be.set_step_control(True)
    prob.bc_values(0.0)
    for k in range(3):
        prob.step((k + 1) * prob.dt, [prob.bcs[3]])
    u, info = prob.state(), be.step_info()
    be.set_step(0.5 * prob.dt)
    prob.step(3.5 * prob.dt, [prob.bcs[3]])
    first, e1 = prob.state(), be.step_error(0.1)
    be.step_reject()
    assert np.array_equal(prob.state(), u) and {k: be.step_info()[k] for k in ("t", "dt_last", "dt_eff")} == {
        k: info[k] for k in ("t", "dt_last", "dt_eff")}
    with pytest.raises(RuntimeError):
        be.step_reject()
    prob.step(3.5 * prob.dt, [prob.bcs[3]])
    assert np.array_equal(prob.state(), first) and be.step_error(0.1) == e1 > 0.0


def test_the_new_calls_are_declared_and_bound():
    names = ["hf_set_step", "hf_set_step_list", "hf_set_step_control", "hf_get_step_error", "hf_step_reject", "hf_get_step_info"]
    for n in names:
        assert n in hip_backend.EXPORTS
    for m in ("set_step", "set_step_list", "set_step_control", "step_error", "step_reject", "step_info"):
        assert callable(getattr(hip_backend.HeatflowHIP, m)) and callable(getattr(VarstepOracleBackend, m))
