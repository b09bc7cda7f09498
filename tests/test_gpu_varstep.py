"""Variable time steps on the GPU (hf_set_step, hf_set_step_list, hf_set_step_control) against the float64
restatement of tests/varstep_oracle.py: the re-valued operator bit for bit, the default path untouched, the fields of a 12-step list
(both meshes, both preconditioners, every start-vector kind, both schemes; with a load, the source, lagged tables), hf_run against
hf_step + hf_set_step, the local-error estimate, rejection, an adaptive run under a smooth pulse, and the error returns.

The list: the issue gives dt * [1, 0.5, 2, 1.7, 0.3, 1, 1, 2.4, 0.6, 1.2, 0.25, 2] and states that every ratio stays below
1 + sqrt 2.  Read as step sizes the numbers have ratios of 4 and 8; read as the ratios themselves they satisfy the statement
(the largest is 2.4), so the steps are dt * cumprod(...): 12 steps of 0.22 dt .. 1.7 dt."""
import functools

import numpy as np
import pytest

import source_oracle as so
from helpers import make_problem, material_tables
from rhoc_T_oracle import einstein_tables
from varstep_oracle import (RATIOS, VarstepOracleBackend, oside_node, pulse, small, smooth_problem, smooth_references,
                            step_list)

from heatflow_amd import stepping

pytestmark = pytest.mark.gpu

FIELD_TOL_K = 1e-4           # the tolerance of test_gpu_time_scheme.py
SOURCE_NAMES, SOURCE_DEPTH, SOURCE_POWER, SOURCE_FWHM = ("p_coupler", "p_ins"), 5.0e-7, 0.5, 1.4e-5


def test_the_list_respects_the_bdf2_limit():
    r = np.cumprod(RATIOS)
    assert (r[1:] / r[:-1]).max() < stepping.BDF2_MAX_RATIO


def _variant(case, variant):
    """(problem keywords, source) of a named variant."""
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    ins = [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")]
    T = 300.0 + 10.0 * np.arange(51)
    ktab = {t: (300.0, 10.0, tk[t] * 300.0 / T) for t in ins}
    if variant == "source":
        tags = [mesh.material_tags[n] for n in SOURCE_NAMES]
        return {"source": {"tags": tags, "fwhm": SOURCE_FWHM, "z0": float(stack.by_name(SOURCE_NAMES[0]).boundaries[0]),
                           "depth": SOURCE_DEPTH}}
    if variant == "tables1":
        return {"kappa_tables": ktab, "rhoc_tables": einstein_tables(trc, ins), "picard": 1}
    if variant == "tables2":
        return {"kappa_tables": ktab, "rhoc_tables": einstein_tables(trc, ins), "picard": 2}
    if variant == "aniso":
        return {"k_aniso": {mesh.material_tags["p_sample"]: (2.0, 0.25)}}
    return {}


def _prepare(prob, variant, case):
    """Load or source amplitudes of a variant; returns run_steps' source_amplitude."""
    if variant == "load":
        ob = VarstepOracleBackend()
        make_problem(*case, backend=ob, scheme=prob.scheme)
        rng = np.random.default_rng(1)
        prob.set_load((ob.M @ (2.0 + rng.random(prob.n))) / prob.dt)      # dt F ~ M (2..3 K) per step
    if variant == "source":
        p0 = so.peak_density(SOURCE_POWER, prob.source_vector())
        return lambda t: p0 * float(pulse(t, 1.2e-6, 1.2e-6))
    return None


def _list_fields(case, scheme, variant, backend=None, precond=0, kind=None):
    prob = make_problem(*case, backend=backend, precond=precond, scheme=scheme, **_variant(case, variant))
    try:
        if kind is not None:
            prob.backend.set_start_vector(kind)
        amp = _prepare(prob, variant, case)
        nodes = np.arange(prob.n, dtype=np.int32)
        _, fields, iters = prob.run_steps(step_list(prob.dt), watcher_nodes=nodes, time_varying=[prob.bcs[3]], source_amplitude=amp)
        info = prob.backend.step_info()
        fb = prob.backend.amg_info()["jacobi_fallbacks"] if backend is None and precond == 1 else 0
        return fields, np.asarray(iters), info, fb
    finally:
        prob.close()


@functools.lru_cache(maxsize=None)
def _reference(which, scheme, variant):
    fields, _, info, _ = _list_fields(small(which), scheme, variant, backend=VarstepOracleBackend())
    fields.setflags(write=False)
    return fields, info


# 1. the operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "aniso", "tables1"])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_revalued_operator_is_bitwise_the_assembled_one(hip, scheme, variant):
    """One step of the assembled size, then hf_set_step(0.37 dt) and one more (BDF2: omega = 0.37): A equals the A of a second
    context assembled at step_info().dt_eff under backward Euler - under tables at the evaluation state of that step - and M is
    unchanged (under capacity tables: the M of that state)."""
    case = small("with_diamond")
    kw = _variant(case, variant)
    prob = make_problem(*case, scheme=scheme, **kw)
    ref = make_problem(*case, scheme="backward_euler", **kw)
    try:
        be = prob.backend
        _, _, _, M0 = be.get_csr()
        u0 = prob.state()
        prob.bc_values(0.0)                                        # every condition at t = 0, as run() sets them
        prob.step(prob.dt, [prob.bcs[3]])
        u1 = prob.state()
        dt2 = 0.37 * prob.dt
        be.set_step(dt2)
        assert be.step_info()["revaluations"] == 0                # lazy: nothing happens before the step
        prob.step(prob.dt + dt2, [prob.bcs[3]])
        info = be.step_info()
        om = dt2 / prob.dt
        want = dt2 if scheme == "backward_euler" else dt2 * (1.0 + om) / (1.0 + 2.0 * om)
        assert info["dt_eff"] == want and info["dt_last"] == dt2 and info["t"] == prob.dt + dt2
        assert info["revaluations"] == 1
        _, _, A, M = be.get_csr()
        if variant == "tables1":
            ref.set_state(u1 if scheme == "backward_euler" else (1.0 + om) * u1 - om * u0)
        ref.backend.assemble(info["dt_eff"], ref.assembly_mode)
        _, _, A_ref, M_ref = ref.backend.get_csr()
        assert np.array_equal(A, A_ref)
        assert np.array_equal(M, M_ref)
        if variant != "tables1":
            assert np.array_equal(M, M0)
        assert np.abs(A - M).max() > 0.0
    finally:
        prob.close()
        ref.close()


# 2. nothing moves by default ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_a_list_of_the_assembled_step_is_bitwise_hf_run(hip, scheme, precond):
    case = small("with_diamond")
    nodes = np.arange(0, len(case[2].coords), 11, dtype=np.int32)
    out = []
    for listed in (False, True):
        prob = make_problem(*case, precond=precond, scheme=scheme)
        try:
            if listed:
                _, s, it = prob.run_steps([prob.dt] * 10, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
                assert prob.backend.step_info()["revaluations"] == 0
            else:
                _, s, it = prob.run(10, watcher_nodes=nodes, time_varying=[prob.bcs[3]])
            out.append((s, np.asarray(it), prob.state()))
        finally:
            prob.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert np.abs(out[0][0][-1] - out[0][0][0]).max() > 0.0


# 3. fields on a list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("which", ["with_diamond", "no_diamond"])
def test_list_fields_match_the_restatement_at_every_step(hip, which, precond, scheme, kind):
    ref, rinfo = _reference(which, scheme, "plain")
    gpu, iters, info, fallbacks = _list_fields(small(which), scheme, "plain", precond=precond, kind=kind)
    worst = float(np.abs(gpu - ref).max())
    print(f"list {which} precond={precond} {scheme} kind={kind}: worst |dT| = {worst:.2e} K, iterations {int(iters.sum())}, "
          f"re-valuations {info['revaluations']}")
    assert worst <= FIELD_TOL_K, f"{worst:.3e} K"
    assert info["t"] == rinfo["t"] and info["dt_eff"] == rinfo["dt_eff"] and info["revaluations"] == rinfo["revaluations"]
    assert fallbacks == 0
    assert np.abs(ref[-1] - ref[0]).max() > 0.0


@pytest.mark.parametrize("variant", ["load", "source", "tables1", "tables2", "aniso"])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
def test_list_fields_of_the_variants_match_the_restatement(hip, precond, scheme, variant):
    ref, _ = _reference("with_diamond", scheme, variant)
    plain, _ = _reference("with_diamond", scheme, "plain")
    gpu, iters, info, fallbacks = _list_fields(small("with_diamond"), scheme, variant, precond=precond)
    worst = float(np.abs(gpu - ref).max())
    moved = float(np.abs(ref - plain).max())
    print(f"list {variant} precond={precond} {scheme}: worst |dT| = {worst:.2e} K, the variant moves the field by {moved:.2e} K, "
          f"iterations {int(iters.sum())}")
    assert worst <= FIELD_TOL_K, f"{worst:.3e} K"
    assert moved > 100.0 * FIELD_TOL_K                      # the variant is really in the run
    if variant in ("load", "source"):
        assert fallbacks == 0


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
def test_hf_run_with_the_list_is_bitwise_hf_step_with_set_step(hip, precond, scheme):
    case = small("with_diamond")
    out = []
    for through_step in (False, True):
        prob = make_problem(*case, precond=precond, scheme=scheme)
        try:
            dts = step_list(prob.dt)
            if through_step:
                prob.bc_values(0.0)
                t, fields = 0.0, []
                for h in dts:
                    t += h
                    prob.backend.set_step(h)
                    prob.step(t, [prob.bcs[3]])
                    fields.append(prob.state())
                out.append(np.array(fields))
            else:
                _, s, _ = prob.run_steps(dts, watcher_nodes=np.arange(prob.n, dtype=np.int32), time_varying=[prob.bcs[3]])
                out.append(s)
        finally:
            prob.close()
    assert np.array_equal(out[0], out[1])


# 4. the estimator --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_step_error_matches_the_float64_formula(hip, scheme):
    """After steps 3, 6 and 9 of the list (and after step 1, where all history is the rest state): hf_get_step_error against the
    formula evaluated in numpy on the GPU's own states, within the rounding bound of the expression,
    8 eps c max_i(|u_i| + sum_k |w_k h_k,i|) / atol_e."""
    case = small("with_diamond")
    prob = make_problem(*case, scheme=scheme)
    atol_e = 0.05
    try:
        be = prob.backend
        be.set_step_control(True)
        prob.bc_values(0.0)
        dts = step_list(prob.dt)
        order = stepping.scheme_order(scheme)
        free = np.ones(prob.n, dtype=bool)
        free[prob.bc_dofs] = False
        states, t = [prob.state()], 0.0
        for k, h in enumerate(dts[:9]):
            t += h
            be.set_step(h)
            prob.step(t, [prob.bcs[3]])
            states.append(prob.state())
            if k + 1 in (1, 3, 6, 9):
                got = be.step_error(atol_e, 0.0)
                d0, d1, d2 = stepping.history_steps(dts[:k + 1])
                hist = states[-2::-1][:3]
                hist = hist + [hist[-1]] * (3 - len(hist))
                wts = stepping.predictor_weights(order, d0, d1, d2)
                c = stepping.estimator_constant(order, d0, d1, d2)
                e, mag = states[-1].copy(), np.abs(states[-1])
                for wk, hk in zip(wts, hist):
                    e = e - wk * hk
                    mag = mag + np.abs(wk * hk)
                want = float(np.abs(c * e[free]).max() / atol_e)
                bound = 8.0 * np.finfo(float).eps * c * float(mag[free].max()) / atol_e
                print(f"estimate {scheme} after step {k + 1}: GPU {got:.6e}, float64 {want:.6e}, |difference| {abs(got - want):.2e}, "
                      f"bound {bound:.2e}")
                assert abs(got - want) <= bound
                if k + 1 >= 3:
                    assert got > 0.0
    finally:
        prob.close()


# 5. rejection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
def test_rejection_restores_the_step_before_bitwise(hip, precond, scheme, kind):
    from heatflow_amd.hip_backend import HF_ERR_STATE, HipError

    case = small("with_diamond")
    kw = _variant(case, "source")
    prob = make_problem(*case, precond=precond, scheme=scheme, monitors={"sample": {"tags": [case[2].material_tags["p_sample"]],
                                                                                    "above": 310.0}}, **kw)
    try:
        be = prob.backend
        be.set_start_vector(kind)
        prob.record_heat(True)
        be.set_step_control(True)
        prob.bc_values(0.0)
        p0 = so.peak_density(SOURCE_POWER, prob.source_vector())
        dts = step_list(prob.dt)
        amps = [p0 * float(pulse(t, 1.2e-6, 1.2e-6)) for t in np.cumsum(dts)]
        t = 0.0
        for k in range(5):
            t += dts[k]
            be.set_step(dts[k])
            be.set_source_amplitudes([amps[k]])
            be.step(prob.bc_values(t, [prob.bcs[3]]), prob.rtol, prob.atol, prob.max_it)
        before = (prob.state(), be.step_info(), be.monitor_count(), be.heat_count())
        for h, undo_twice in ((dts[5], True), (0.4 * dts[5], False)):      # the size before continues; a new one re-values
            be.set_step(h)
            be.set_source_amplitudes(amps[5:7])            # two entries: the redone step must take the first one again
            g = prob.bc_values(t + h, [prob.bcs[3]])
            be.step(g, prob.rtol, prob.atol, prob.max_it)
            first = prob.state()
            assert np.abs(first - before[0]).max() > 0.0
            assert be.monitor_count() == before[2] + 1 and be.heat_count() == before[3] + 1
            be.step_reject()
            info = be.step_info()
            assert np.array_equal(prob.state(), before[0])
            assert (info["t"], info["dt_last"], info["dt_eff"]) == (before[1]["t"], before[1]["dt_last"], before[1]["dt_eff"])
            assert be.monitor_count() == before[2] and be.heat_count() == before[3]
            if undo_twice:
                with pytest.raises(HipError) as e:
                    be.step_reject()
                assert e.value.code == HF_ERR_STATE and "hf_step_reject" in str(e.value)
            be.step(g, prob.rtol, prob.atol, prob.max_it)            # the same size again: the first attempt's bits
            assert np.array_equal(prob.state(), first)
            be.step_reject()
        # the history is the one of before too: the next two steps equal those of a run that never tried
        be.set_step(dts[5])
        be.set_source_amplitudes(amps[5:7])
        for k in (5, 6):
            t += dts[k]
            be.set_step(dts[k])
            be.step(prob.bc_values(t, [prob.bcs[3]]), prob.rtol, prob.atol, prob.max_it)
        after = prob.state()
    finally:
        prob.close()
    plain = make_problem(*case, precond=precond, scheme=scheme, **kw)
    try:
        plain.backend.set_start_vector(1)
        _, s, _ = plain.run_steps(dts[:7], watcher_nodes=np.arange(plain.n, dtype=np.int32), time_varying=[plain.bcs[3]],
                                  source_amplitude=amps[:7])
    finally:
        plain.close()
    assert np.abs(after - s[-1]).max() <= FIELD_TOL_K
    if kind == 1:
        assert np.array_equal(after, s[-1])


# 6. the adaptive run -----------------------------------------------------------------------------------------------------------
def test_adaptive_run_under_a_smooth_pulse(hip):
    """BDF2, tol 0.1 K, 30 us: every accepted step's field on the GPU against the replay of the accepted sizes on the restatement
    (the same consistent start), the o-side error against 6400 fixed steps of the restatement, the count of solves; and the
    assembled step is in force again afterwards."""
    case = small("with_diamond")
    node = int(oside_node(case)[0])
    (t_ref, o_ref), err800 = smooth_references()
    prob = smooth_problem(case, precond=1, scheme="bdf2")
    try:
        every = np.arange(prob.n, dtype=np.int32)
        times, s, iters, info = prob.run_adaptive(3.0e-5, 0.1, watcher_nodes=every, time_varying=[prob.bcs[3]])
        n_iter = int(np.sum(prob.iters))
        t_after, _, _ = prob.run(2, time_varying=[prob.bcs[3]], first_step=0)          # (boundary values of (k+1) dt: only the sizes matter)
        after = prob.backend.step_info()
    finally:
        prob.close()
    assert times[-1] == 3.0e-5 and info["accepted"] == len(times) == len(info["dt"])
    assert after["dt_last"] == prob.dt
    err = float(np.abs(s[:, node] - np.interp(times, t_ref, o_ref)).max())
    solves = info["accepted"] + info["rejected"]
    rest = smooth_problem(case, backend=VarstepOracleBackend(), scheme="bdf2")
    tr, sr, _ = rest.run_steps(info["dt"], watcher_nodes=every, time_varying=[rest.bcs[3]], consistent_start=True)
    per_step = np.abs(sr - s).max(axis=1)
    print(f"adaptive BDF2 tol 0.1 K: {info['accepted']} + {info['rejected']} solves, {info['revaluations']} re-valuations, steps "
          f"{info['dt'].min():.2e} .. {info['dt'].max():.2e} s, o-side error {err:.4f} K (800 fixed steps: {err800:.4f} K), PCG iterations "
          f"{n_iter}, replay on the restatement: worst |dT| over all steps {per_step.max():.2e} K (step {int(per_step.argmax())}), "
          f"peak rise {float(s.max()) - 300.0:.1f} K")
    assert np.abs(tr - times).max() <= 1e-18
    assert float(s.max()) - 300.0 > 400.0                   # the pulse is in the compared fields
    assert per_step.max() <= FIELD_TOL_K
    assert err <= err800
    assert solves <= 400


# 7. error returns --------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_call(hip):
    from heatflow_amd.hip_backend import HF_ERR_ARG, HF_ERR_STATE, HipError

    case = small("with_diamond")
    lib = hip.load_library()
    prob = make_problem(*case, scheme="bdf2")
    be = prob.backend
    try:
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert lib.hf_set_step(be._ctx, bad) == HF_ERR_ARG
            with pytest.raises(ValueError, match="hf_set_step_list"):
                be.set_step_list([prob.dt, bad])
        # the ratio limit of BDF2: at the call once a history exists, and for every entry of a list before any launch
        prob.step(prob.dt, [prob.bcs[3]])
        with pytest.raises(ValueError, match=r"hf_set_step.*1 \+ sqrt 2"):
            be.set_step(2.5 * prob.dt)
        be.set_step(2.4 * prob.dt)
        be.set_step_list([prob.dt, 2.5 * prob.dt])
        u = prob.state()
        g = prob.bc_values(prob.dt, [prob.bcs[3]])
        with pytest.raises(ValueError, match=r"hf_run.*1 \+ sqrt 2"):
            be.run(np.array([g, g]))
        # a list too short for the run
        be.set_step_list([prob.dt])
        with pytest.raises(HipError) as e:
            be.run(np.array([g, g]))
        assert e.value.code == HF_ERR_STATE and "hf_run" in str(e.value) and "hf_set_step_list" in str(e.value)
        assert np.array_equal(prob.state(), u)            # nothing was launched
        be.set_step_list([])
        # step control: at rest only; estimate and rejection need a step
        with pytest.raises(HipError) as e:
            be.set_step_control(True)
        assert e.value.code == HF_ERR_STATE and "hf_set_step_control" in str(e.value)
        prob.set_state(300.0)
        for call in (lambda: be.step_error(1.0), be.step_reject):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == HF_ERR_STATE
        be.set_step_control(True)
        for call in (lambda: be.step_error(1.0), be.step_reject):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == HF_ERR_STATE
        prob.step(prob.dt, [prob.bcs[3]])
        with pytest.raises(ValueError, match="hf_get_step_error"):
            be.step_error(0.0, 0.0)
        be.set_step_control(False)
        # an open batch and a tangent set-up refuse the calls, and variable steps refuse them
        for call, name in ((lambda: be.batch_begin(2), "hf_batch_begin"),
                           (lambda: prob.run_tangent(1, [0], conductivity=[[case[2].material_tags["p_sample"]]]), "hf_run_tangent")):
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == HF_ERR_STATE and name in str(e.value)
        be.assemble(prob.dt, prob.assembly_mode)          # ends the variable steps
        for name, call in (("hf_set_step", lambda: be.set_step(prob.dt)), ("hf_set_step_list", lambda: be.set_step_list([prob.dt])),
                           ("hf_set_step_control", lambda: be.set_step_control(True))):
            be.batch_begin(2)
            with pytest.raises(HipError) as e:
                call()
            assert e.value.code == HF_ERR_STATE and name in str(e.value) and "batch" in str(e.value)
            be.batch_end()
        be.tangent_setup(1, {case[2].material_tags["p_sample"]: 0})
        with pytest.raises(HipError) as e:
            be.set_step(prob.dt)
        assert e.value.code == HF_ERR_STATE and "tangent" in str(e.value)
    finally:
        prob.close()
    # the enthalpy form, another assembly mode, and a context that is not assembled
    tk, trc = material_tables(case[1], case[2])
    ins = [case[2].material_tags[m.name] for m in case[1].materials if m.name.endswith("ins")]
    prob = make_problem(*case, rhoc_tables=einstein_tables(trc, ins), capacity_form="enthalpy", picard=4)
    try:
        with pytest.raises(HipError) as e:
            prob.backend.set_step(prob.dt)
        assert e.value.code == HF_ERR_STATE and "hf_set_step" in str(e.value) and "enthalpy" in str(e.value)
        with pytest.raises(ValueError, match="enthalpy"):
            prob.run_steps([prob.dt])
    finally:
        prob.close()
    prob = make_problem(*case, assembly_mode=hip.ASM_LDS_COLORED)
    try:
        with pytest.raises(HipError) as e:
            prob.backend.set_step(prob.dt)
        assert e.value.code == HF_ERR_STATE and "row-gather" in str(e.value)
        prob.backend.set_time_scheme(1)
        with pytest.raises(HipError) as e:
            prob.backend.set_step(prob.dt)
        assert e.value.code == HF_ERR_STATE and "hf_assemble" in str(e.value)
    finally:
        prob.close()
