"""Tangent runs under the laser-power source on the GPU (hf_source_derivatives, hf_tangent_set_source, k_source_load_d,
kb_source_columns) against the float64 restatement of tests/source_tangent_oracle.py: the derivative vectors row
by row, the load with source columns among conductivity and capacity columns, the exact recursion, linearity in the power, central
differences of GPU primal runs, the bitwise primal, every error and state rule, and the session, the monitor bands and the fit."""
import copy
import functools
import json
import math

import numpy as np
import pytest

import source_oracle as so
import source_tangent_oracle as sto
from conftest import build_case, load_cfg

pytestmark = pytest.mark.gpu

CASES = {"with_diamond": "geballe_with_diamond", "no_diamond": "geballe_no_diamond"}
KEPT = dict(names=("p_coupler", "p_ins"), depth=5.0e-7, power=0.5)      # tests/test_gpu_source.py's KEPT_LINE_*
KEY = {"source.power": "power", "source.fwhm": "fwhm", "source.depth": "depth", "source.pulse.t0": "t0", "source.pulse.fwhm": "w"}
NSTEPS = sto.NSTEPS


@functools.lru_cache(maxsize=None)
def small(which):
    return build_case(CASES[which], 8.0)


def _tags(case, P):
    return [case[2].material_tags[n] for n in P["names"]]


# 1. the derivative vectors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(names=("p_coupler",), depth=2.0e-8), dict(names=("p_coupler", "p_ins"), depth=5.0e-7)])
@pytest.mark.parametrize("which", sorted(CASES))
def test_derivative_vectors_match_the_restatement_row_by_row(hip, which, kw):
    """|G_i - ref_i| <= 1e-13 sum_j |M1_ij| g_j, the bound of test_source_vector_matches_the_restatement: the same arithmetic plus
    three multiplications per node."""
    case = small(which)
    _, _, mesh = case
    P = sto.beam(case, **kw)
    tags = _tags(case, P)
    Gf, Tf, Gd, Td = sto.derivative_vectors(mesh.coords, mesh.tris, mesh.tags, tags, P["fwhm"], P["z0"], P["depth"])
    with hip.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_source(tags, P["fwhm"], P["z0"], P["depth"])
        F1 = be.get_source()
        be.source_derivatives(True)
        got_f, got_d = be.get_source_derivative(0), be.get_source_derivative("depth")
        assert np.array_equal(be.get_source(), F1)                         # F1 is not touched
        be.set_source(tags, P["fwhm"], P["z0"], math.inf)                  # a uniform layer
        be.source_derivatives(True)
        uni_f, uni_d = be.get_source_derivative(0), be.get_source_derivative(1)
    touched = np.zeros(len(mesh.coords), dtype=bool)
    touched[np.asarray(mesh.tris)[np.isin(mesh.tags, tags)].ravel()] = True
    for name, got, ref, T in (("G_f", got_f, Gf, Tf), ("G_d", got_d, Gd, Td)):
        live = T > 0.0
        ratio = float((np.abs(got - ref)[live] / T[live]).max())
        print(f"{name} {which} {P['names']} depth={P['depth']}: worst |G - ref| / sum |M1| g = {ratio:.2e}, sum = {got.sum():.6e}")
        assert np.all(np.abs(got - ref) <= 1e-13 * T), ratio
        assert live.sum() > 100 and np.abs(ref).max() > 0.0
        assert np.all(got[~touched] == 0.0) and not np.signbit(got[~touched]).any()
    assert not uni_d.any() and not np.signbit(uni_d).any() and uni_f.any()      # G_d of a uniform layer: exact zeros


def test_two_calls_and_two_contexts_give_the_same_bits(hip):
    case = small("with_diamond")
    _, _, mesh = case
    P = sto.beam(case, **KEPT)
    out = []
    for _ in range(2):
        with hip.HeatflowHIP() as be:
            be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
            be.set_source(_tags(case, P), P["fwhm"], P["z0"], P["depth"])
            be.source_derivatives(True)
            first = [be.get_source_derivative(0), be.get_source_derivative(1)]
            be.source_derivatives(True)                                   # the same context again
            for a, w in zip(first, (0, 1)):
                assert np.array_equal(a, be.get_source_derivative(w)) and a.any()
            out.append(first)
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# 2. the load -------------------------------------------------------------------------------------------------------------------------
def _load_columns(mesh, P, nv):
    """(conductivity, capacity, {column: source parameter}) of the load test.  nv = 2: p_sample's k next to source.fwhm alone;
    nv = 16: source.power, source.fwhm on top of p_ins's k, and source.depth in columns 5, 9 and 15, p_sample's k in 0 and
    p_ins's rho_c in 3."""
    t = mesh.material_tags
    if nv == 2:
        return [[t["p_sample"]], []], None, {1: "source.fwhm"}
    cond = [[] for _ in range(16)]
    cap = [[] for _ in range(16)]
    cond[0], cond[9], cap[3] = [t["p_sample"]], [t["p_ins"]], [t["p_ins"]]
    return cond, cap, {5: "source.power", 9: "source.fwhm", 15: "source.depth"}


def _three_steps(prob, P, cond, cap, cols, with_table=True):
    """Three tangent steps, one call each, the pulse at its peak; returns the four states and the last step's coefficients."""
    F1, Gf, Gd = prob.source_vector(), prob.source_derivative("fwhm"), prob.source_derivative("depth")
    states, last = [prob.state()], None
    for k in range(3):
        times = (np.arange(k, k + 1) + 1) * prob.dt
        table = sto.coefficient_table(P["power"], P["t0"], P["w"], times, F1, Gf, Gd)
        source = {j: {"amplitude": table[nm][:, 0], "fwhm": table[nm][:, 1], "depth": table[nm][:, 2]} for j, nm in cols.items()}
        prob.run_tangent(1, None, conductivity=cond, time_varying=[], first_step=k, source=source if with_table else {},
                         source_amplitude=sto.amplitudes(P, times, F1), **({"capacity": cap} if cap else {}))
        states.append(prob.state())
        last = {j: table[nm][0] for j, nm in cols.items()}
    return states, last, (F1, Gf, Gd)


@pytest.mark.parametrize("nv", [2, 16])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_load_after_three_steps_row_by_row(hip, scheme, nv):
    """hf_tangent_load against the restated c0 F1 + c1 G_f + c2 G_d - the restated vectors and the table made from them, and
    again with the GPU's own vectors and coefficients - plus the restated conductivity and capacity parts at the GPU's own
    states: every row within 1e-13 of its sum of absolute terms (for the restated vectors: of the terms of their own row sums).
    Columns without a source part keep the bits of the run without hf_tangent_set_source, and the source.fwhm column's source
    part carries no net power."""
    case = small("with_diamond")
    _, _, mesh = case
    P = sto.beam(case, names=("p_coupler", "p_ins"), depth=5.0e-7, power=0.5, t0_steps=2.0, w_steps=4.0)
    cond, cap, cols = _load_columns(mesh, P, nv)
    loads = {}
    for with_table in (True, False):
        prob = sto.problem(case, P, False, precond=1, scheme=scheme)
        try:
            states, last, (F1, Gf, Gd) = _three_steps(prob, P, cond, cap, cols, with_table)
            assert prob.backend.tangent_nv == nv
            loads[with_table] = (states, [prob.tangent_load(j) for j in range(nv)])
        finally:
            prob.close()
    (states, got), (states0, plain) = loads[True], loads[False]
    for a, b in zip(states, states0):
        assert np.array_equal(a, b)                                         # the primal does not see the table
    for j in range(nv):
        if j not in cols:
            assert np.array_equal(got[j], plain[j]), j                      # unmasked columns keep their bits
    assert plain[0].any() and (nv == 2 or plain[3].any())
    # the other parts, restated at the GPU's states
    ref = sto.problem(case, P, False, backend=sto.SourceTangentOracleBackend(), scheme=scheme)
    _three_steps(ref, P, cond, cap, cols, False)
    # the source part, restated from the mesh alone: the vectors, their rows' sums of absolute terms, and the table of step 3
    tags = _tags(case, P)
    rF1, sF1 = so.source_vector(mesh.coords, mesh.tris, mesh.tags, tags, P["fwhm"], P["z0"], P["depth"])
    rGf, sGf, rGd, sGd = sto.derivative_vectors(mesh.coords, mesh.tris, mesh.tags, tags, P["fwhm"], P["z0"], P["depth"])
    rtable = sto.coefficient_table(P["power"], P["t0"], P["w"], [3 * ref.dt], rF1, rGf, rGd)
    worst = worst_r = 0.0
    for j, c in last.items():
        other, T0 = ref.backend.tangent_load_terms(j, state=(states[3], states[2], states[1]))
        r = rtable[cols[j]][0]
        for label, cc, (v0, v1, v2), (a0, a1, a2) in (("gpu", c, (F1, Gf, Gd), (np.abs(F1), np.abs(Gf), np.abs(Gd))),
                                                      ("restated", r, (rF1, rGf, rGd), (sF1, sGf, sGd))):
            src = (cc[0] * v0 + cc[1] * v1) + cc[2] * v2
            T = T0 + (abs(cc[0]) * a0 + abs(cc[1]) * a1) + abs(cc[2]) * a2
            want = other + src
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(T > 0, np.abs(got[j] - want) / T, np.where(got[j] == 0, 0.0, np.inf))
            if label == "gpu":
                worst = max(worst, float(ratio.max()))
            else:
                worst_r = max(worst_r, float(ratio.max()))
            assert np.abs(src).max() > 0.0
        assert not np.array_equal(got[j], plain[j])
        assert np.array_equal(got[j][rF1 == 0.0], plain[j][rF1 == 0.0])     # only the source's rows are touched
    print(f"{scheme} nv={nv}: max |F - ref| / sum of absolute terms = {worst_r:.2e} (restated vectors and table), {worst:.2e} "
          f"(the GPU's own vectors)")
    assert worst_r <= 1e-13 and worst <= 1e-13
    if nv == 2:       # a column with the source part alone: it sums to zero, the configured power staying the discrete power
        c = last[1]
        total = math.fsum(got[1])
        scale = math.fsum(np.abs(c[0] * F1)) + math.fsum(np.abs(c[1] * Gf))
        print(f"{scheme}: sum of the source.fwhm column's load = {total:.3e}, sum of absolute terms {scale:.3e}")
        assert not plain[1].any() and abs(total) <= 1e-13 * scale


# 3. the exact recursion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_line", [False, True])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("which", sorted(CASES))
def test_tangents_match_the_exact_recursion(hip, which, scheme, keep_line):
    case = small(which)
    _, _, mesh = case
    nodes = np.sort(np.random.default_rng(0).choice(len(mesh.coords), 12, replace=False)).astype(np.int32)
    P = sto.beam(case, **(KEPT if keep_line else {}))

    def run(**kw):
        prob = sto.problem(case, P, keep_line, scheme=scheme, **kw)
        try:
            names, _, _, ts, _ = sto.tangent_run(prob, case, P, nodes, keep_line=keep_line)
            return names, ts, [prob.tangent(j) for j in range(len(names))]
        finally:
            prob.close()

    names, ts_ref, f_ref = run(backend=sto.SourceTangentOracleBackend())
    assert names[:2] == ["p_sample", "p_sample.rho_c"] and set(sto.SOURCE_PARAMS) <= set(names) and (names[-1] == "fwhm") == keep_line
    for precond in (0, 1):
        _, ts, fields = run(precond=precond)
        for j, nm in enumerate(names):
            scale = np.max(np.abs(f_ref[j]))
            assert scale > 0
            err_s, err_f = np.max(np.abs(ts[:, j] - ts_ref[:, j])) / scale, np.max(np.abs(fields[j] - f_ref[j])) / scale
            print(f"{which} {scheme} keep_line={keep_line} precond={precond} {nm}: samples off by {err_s:.2e}, final field by "
                  f"{err_f:.2e} of max|s|")
            assert err_s <= 1e-6 and err_f <= 1e-6, (which, scheme, keep_line, precond, nm)


# 4. linearity in the power: exact, no finite difference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_the_power_column_is_the_rise_over_the_power(hip, scheme):
    """Outer edges at ic_temp, no heated line: u - ic_temp is linear in P, so d u / d P = (u - ic_temp) / P at every node and step,
    and over a region that covers the whole cell d energy / d P = energy / P; both to 1e-6 of their maxima, the margin of two
    solves at the default rtol."""
    case = small("with_diamond")
    _, _, mesh = case
    P = sto.beam(case)
    nodes = np.arange(len(mesh.coords), dtype=np.int32)
    every = sorted(set(int(t) for t in mesh.tags))
    prob = sto.problem(case, P, False, precond=1, scheme=scheme, monitors={"cell": {"tags": every, "above": None}})
    try:
        names, _, s, ts, _ = sto.tangent_run(prob, case, P, nodes, monitor_tangents=True)
        j = names.index("source.power")
        energy = prob.monitor_history()["cell"]["energy"]
        d_energy = prob.monitor_tangent_history()["cell"]["energy"][:, j]
    finally:
        prob.close()
    want = (s - 300.0) / P["power"]
    scale = float(np.abs(want).max())
    err = float(np.abs(ts[:, j] - want).max())
    e_err = float(np.abs(d_energy - energy / P["power"]).max() / np.abs(energy / P["power"]).max())
    print(f"{scheme}: peak rise {s.max() - 300.0:.1f} K, |s_P - (u - ic) / P| / max = {err / scale:.2e}, |dE/dP - E / P| / max = {e_err:.2e}")
    assert s.max() - 300.0 >= 10.0 and err <= 1e-6 * scale
    assert energy.max() > 0.0 and e_err <= 1e-6


# 5. central differences of GPU primal runs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["source.fwhm", "source.depth"])
def test_tangents_match_central_differences_of_gpu_runs(hip, name):
    """Multigrid at rtol = 1e-12; the relative step is the one tests/test_source_tangent_cpu.py found in float64."""
    case = small("with_diamond")
    _, _, mesh = case
    nodes = np.arange(0, len(mesh.coords), max(1, len(mesh.coords) // 50), dtype=np.int32)
    P = sto.beam(case, **KEPT)                                              # (a depth the field feels: 0.5 um over two layers)
    rel, theta0 = sto.FD_REL_STEP[name], P[KEY[name]]
    prob = sto.problem(case, P, False, precond=1, rtol=1e-12)
    try:
        names, _, _, ts, _ = sto.tangent_run(prob, case, P, nodes)
        s = ts[:, names.index(name)]
    finally:
        prob.close()
    runs = []
    for sg in (1.0, -1.0):
        Q = dict(P, **{KEY[name]: theta0 * (1.0 + sg * rel)})
        prob = sto.problem(case, Q, False, precond=1, rtol=1e-12)
        try:
            runs.append(sto.primal_run(prob, Q, nodes)[1])
        finally:
            prob.close()
    fd = (runs[0] - runs[1]) / (2.0 * rel * theta0)
    scale, err = float(np.max(np.abs(s))), float(np.max(np.abs(s - fd)))
    print(f"{name}: max |s| theta = {scale * theta0:.3e} K; |s - FD| / max|s| = {err / scale:.2e} at relative step {rel:g}")
    assert scale > 0 and err <= 1e-4 * scale


# 6. the primal ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("monitors", [False, True])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_primal_under_a_source_is_bitwise_that_of_hf_run(hip, scheme, monitors):
    case = small("with_diamond")
    _, _, mesh = case
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    P = sto.beam(case, **KEPT)
    kw = {"monitors": {"coupler": {"tags": [mesh.material_tags["p_coupler"]], "above": 320.0}}} if monitors else {}
    for precond in (0, 1):
        out = []
        for tangent in (False, True):
            prob = sto.problem(case, P, True, precond=precond, scheme=scheme, **kw)
            try:
                if tangent:
                    _, _, s, _, it = sto.tangent_run(prob, case, P, nodes, keep_line=True, monitor_tangents=monitors)
                else:
                    _, s, it = sto.primal_run(prob, P, nodes, keep_line=True)
                rec = prob.backend.get_monitors() if monitors else np.zeros(0)
                out.append((s, it, prob.state(), rec))
            finally:
                prob.close()
        for a, b in zip(*out):
            assert np.array_equal(a, b), precond
        assert out[0][0].max() - 300.0 >= 10.0


# 7. errors and state rules -----------------------------------------------------------------------------------------------------------------
def _state_error(hip, fn, pattern):
    with pytest.raises(hip.HipError, match=pattern) as ei:
        fn()
    assert ei.value.code == hip.HF_ERR_STATE


def test_error_returns_and_state_rules(hip):
    case = small("with_diamond")
    _, _, mesh = case
    P = sto.beam(case)
    tag = mesh.material_tags["p_coupler"]
    prob = sto.problem(case, P, True, precond=0)
    be = prob.backend
    try:
        g = prob.bc_values(prob.dt)
        be.set_source(None)
        _state_error(hip, lambda: be.source_derivatives(True), "hf_source_derivatives: no source set")
        _state_error(hip, lambda: be.source_derivatives(False), "hf_source_derivatives: no source set")
        _state_error(hip, lambda: be.get_source_derivative(0), "hf_get_source_derivative: the source is not differentiable")
        be.set_source([tag], P["fwhm"], P["z0"], P["depth"])
        _state_error(hip, lambda: be.get_source_derivative(0), "hf_get_source_derivative: the source is not differentiable")
        _state_error(hip, lambda: be.tangent_setup(1, {tag: 0}), "hf_tangent_setup: a source is set")
        # the switch opens all three calls; hf_set_source, setting or clearing, closes them again
        be.source_derivatives(True)
        with pytest.raises(ValueError, match=r"hf_get_source_derivative: which = 2"):
            be.get_source_derivative(2)
        be.tangent_setup_dir(1, r={tag: 0})
        be.tangent_setup(3, {tag: 0})
        be.set_source_amplitudes([])
        be.run_tangent(np.stack([g]))
        be.source_derivatives(False)
        _state_error(hip, lambda: be.run_tangent(np.stack([g])), "hf_run_tangent: a source is set")
        _state_error(hip, lambda: be.tangent_set_source(np.ones((1, 4, 3))), "hf_tangent_set_source: the source is not differentiable")
        be.source_derivatives(True)
        be.set_source([tag], P["fwhm"], P["z0"], P["depth"])
        _state_error(hip, lambda: be.tangent_setup(1, {tag: 0}), "hf_tangent_setup: a source is set")
        _state_error(hip, lambda: be.tangent_setup_dir(1, r={tag: 0}), "hf_tangent_setup_dir: a source is set")
        _state_error(hip, lambda: be.run_tangent(np.stack([g])), "hf_run_tangent: a source is set")
        _state_error(hip, lambda: be.get_source_derivative(1), "the source is not differentiable")
        be.source_derivatives(True)
        # the table: its shape, its entries, its length against the run
        be.tangent_setup(3, {tag: 0})
        with pytest.raises(ValueError, match=r"coef must be \(n_steps, 4, 3\)"):
            be.tangent_set_source(np.ones((2, 3, 3)))
        bad = np.zeros((2, 4, 3))
        bad[1, 2, 1] = math.nan
        with pytest.raises(ValueError, match="hf_tangent_set_source: the coefficient of step 1, column 2 is not finite"):
            be.tangent_set_source(bad)
        coef = np.zeros((2, 4, 3))
        coef[:, 1, 0] = 1.0e9
        be.tangent_set_source(coef)
        u0, s0 = be.get_state(), be.get_tangent(1)
        _state_error(hip, lambda: be.run_tangent(np.stack([g, g, g])), r"hf_run_tangent: the source columns have 2 rows left for 3 steps")
        assert np.array_equal(be.get_state(), u0) and np.array_equal(be.get_tangent(1), s0)      # a refused call changes nothing
        assert not be.tangent_load(1).any()                               # nothing before a step
        be.run_tangent(np.stack([g, g]))
        assert be.tangent_load(1).any() and be.get_tangent(1).any() and not be.get_tangent(2).any()
        _state_error(hip, lambda: be.run_tangent(np.stack([g])), r"hf_run_tangent: the source columns have 0 rows left for 1 steps")
        be.tangent_set_source(None)                                        # n_steps = 0 removes the columns
        be.run_tangent(np.stack([g]))
        assert not be.tangent_load(1).any()
        be.tangent_set_source(coef)
        be.tangent_setup(3, {tag: 0})                                      # either set-up removes the table
        be.run_tangent(np.stack([g, g, g]))
        assert not be.get_tangent(1).any()
        # the amplitudes' list binds hf_run_tangent as it binds hf_run
        be.set_source_amplitudes([0.0])
        _state_error(hip, lambda: be.run_tangent(np.stack([g, g])), r"hf_run_tangent: the source has 1 amplitudes left for 2 steps")
        be.set_source_amplitudes([])
        # a shape column under a source: refused by the run, with a message that names both
        be.tangent_set_shape(0, np.zeros(prob.n))
        _state_error(hip, lambda: be.run_tangent(np.stack([g])), r"hf_run_tangent: a source is set and a column has a shape part")
        be.tangent_set_shape(0, None)
        be.run_tangent(np.stack([g]))
        # the refusals that stay: a load, a batch
        be.set_load(np.zeros(prob.n))
        _state_error(hip, lambda: be.run_tangent(np.stack([g])), "hf_run_tangent: a load is set")
        _state_error(hip, lambda: be.tangent_setup(1, {tag: 0}), "hf_tangent_setup: a load is set")
        be.set_load(None)
        _state_error(hip, lambda: be.batch_begin(2), "hf_batch_begin: a source is set")
        # no set-up: the table has nothing to belong to
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        _state_error(hip, lambda: be.tangent_set_source(np.ones((1, 2, 3))), "hf_tangent_set_source before hf_tangent_setup")
        _state_error(hip, lambda: be.source_derivatives(True), "hf_source_derivatives: no source set")
    finally:
        prob.close()


def test_tables_and_the_steady_state_stay_refused_under_a_differentiable_source(hip):
    """The refusals that stay once hf_source_derivatives is on: conductivity or capacity tables (both set-ups and the run) and a
    state that comes from hf_steady_solve (the run), each HF_ERR_STATE with the message of before, state and tangents untouched."""
    from helpers import material_tables

    case = small("with_diamond")
    _, stack, mesh = case
    P = sto.beam(case, **KEPT)
    tag = mesh.material_tags["p_sample"]
    tk, trc = material_tables(stack, mesh)
    prob = sto.problem(case, P, True, precond=1, max_it=400000)
    be = prob.backend
    try:
        g = np.stack([prob.bc_values((k + 1) * prob.dt) for k in range(3)])
        be.source_derivatives(True)
        be.tangent_setup(2, {tag: 0})
        coef = np.zeros((3, 2, 3))
        coef[:, 1, 0] = 1.0e9
        be.tangent_set_source(coef)
        be.set_source_amplitudes([1.0e12] * 3)
        be.run_tangent(g)                                                 # a state and tangents that a refused call could spoil
        for setter, value, what in ((be.set_kappa_tables, tk[tag], r"kappa\(T\)"), (be.set_rhoc_tables, trc[tag], r"rho_c\(T\)")):
            setter({tag: (250.0, 50.0, [value] * 4)})
            u0, s0, s1 = be.get_state(), be.get_tangent(0), be.get_tangent(1)
            assert s0.any() and s1.any()
            _state_error(hip, lambda: be.tangent_setup(2, {tag: 0}), rf"hf_tangent_setup: {what} tables are set")
            _state_error(hip, lambda: be.tangent_setup_dir(2, r={tag: 0}), rf"hf_tangent_setup_dir: {what} tables are set")
            _state_error(hip, lambda: be.run_tangent(g[:1]), rf"hf_run_tangent: {what} tables are set")
            assert np.array_equal(be.get_state(), u0) and np.array_equal(be.get_tangent(0), s0) and np.array_equal(be.get_tangent(1), s1)
            setter({})                                                    # cleared: the constant coefficients again
            be.assemble(prob.dt, prob.assembly_mode)
            be.tangent_setup(2, {tag: 0})
            be.tangent_set_source(coef)
            be.set_source_amplitudes([1.0e12] * 3)
            be.run_tangent(g)
        # the steady state depends on the conductivities, and the tangents start at zero: refused until hf_set_state
        prob.solve_steady(t=3 * prob.dt)
        be.set_source_amplitudes([])
        u0, s0 = be.get_state(), be.get_tangent(1)
        _state_error(hip, lambda: be.run_tangent(g[:1]), "hf_run_tangent: the state comes from hf_steady_solve")
        assert np.array_equal(be.get_state(), u0) and np.array_equal(be.get_tangent(1), s0)
        be.set_state(u0)
        be.tangent_set_source(coef)                                       # (the run before used the table's three rows up)
        be.run_tangent(g[:1])
    finally:
        prob.close()


# 8. the session, the bands and the fit --------------------------------------------------------------------------------------------------------
def _session_cfg(monitors=True):
    cfg = copy.deepcopy(load_cfg("geballe_with_diamond"))
    cfg["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in cfg["mats"].items()}
    cfg["heating"]["source"] = {"material": "p_coupler", "power": 0.2, "fwhm": sto.FWHM, "depth": 2.0e-8,
                                "pulse": {"t0": 7.5e-7, "fwhm": 6.0e-7}, "tangents": True}
    cfg["timing"] = dict(cfg["timing"], num_steps=NSTEPS, t_final=NSTEPS * 7.5e-8)
    if monitors:
        cfg["monitors"] = {"coupler": {"material": "p_coupler", "above": 320.0}, "sample": {"material": "p_sample"}}
    return cfg


def test_session_tangents_and_monitor_bands(hip, tmp_path):
    import csv

    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.run_with_diamond import run_simulation

    cfg = _session_cfg()
    names = ["p_sample", "p_sample.rho_c"] + list(sto.SOURCE_PARAMS)
    sigma = {"source.power": 0.05, "source.fwhm": 0.1, "p_sample.rho_c": 0.15}
    out = tmp_path / "out"
    res = run_simulation(cfg, str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=str(out), tangents=names,
                         monitor_sigma=sigma, watcher_points=get_watcher_points(cfg), write_xdmf=False, suppress_print=True)
    assert list(res["tangents"]) == names
    for nm in names:
        for w in ("pside", "oside"):
            curve = res["tangents"][nm][w]
            assert np.all(np.isfinite(curve)) and np.abs(curve).max() > 0.0, (nm, w)
    band = res["monitor_uncertainty"]["coupler"]["T_max"]
    assert np.all(np.isfinite(band)) and band.max() > 0.0
    with open(out / "monitor_uncertainty.csv", newline="") as f:
        rows = list(csv.reader(f))
    col = rows[0].index("coupler.T_max.sigma")
    written = np.array([float(r[col]) for r in rows[1:]])
    assert len(written) == NSTEPS and np.all(np.isfinite(written)) and np.count_nonzero(written) >= NSTEPS - 1
    assert np.array_equal(written, np.asarray(band))
    print(f"coupler.T_max peaks at {res['monitors']['coupler']['T_max'].max():.1f} K, its one-sigma band at {band.max():.2f} K")


def test_fit_recovers_p_sample_under_a_source_with_a_nuisance_budget(hip, tmp_path):
    import yaml

    from heatflow_amd import fit
    from heatflow_amd.driver import SimulationSession, prepare_mesh
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    cfg = _session_cfg(monitors=False)
    k0 = float(cfg["mats"]["p_sample"]["k"])
    folder = tmp_path / "mesh"
    mesh = prepare_mesh(cfg, str(folder), True, build_stack(cfg))
    s = SimulationSession(*mesh)
    try:
        c = fit.set_params(cfg, ("p_sample",), [1.1 * k0])
        res = s.run(c, build_stack(c), get_watcher_points(c))
    finally:
        s.close()
    with open(tmp_path / "exp.csv", "w") as f:
        f.write("time,temp,oside\n")
        for t, p, o in zip(res["times"], res["watchers"]["pside"], res["watchers"]["oside"]):
            f.write(f"{float(t)!r},{float(p)!r},{float(o)!r}\n")
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    assert fit.main(["--config", str(tmp_path / "cfg.yaml"), "--params", "p_sample", "--exp-csv", str(tmp_path / "exp.csv"),
                     "--mesh-folder", str(folder), "--output-dir", str(tmp_path / "fit"), "--max-iter", "10",
                     "--nuisance", "source.fwhm=0.1", "source.depth=0.2"]) == 0
    with open(tmp_path / "fit" / "fit_summary.json") as f:
        out = json.load(f)
    print(f"fit under a source: {out['values']} in {out['iterations']} iterations, {out['runs']} runs; systematic {out['systematic']}")
    assert abs(out["values"][0] / (1.1 * k0) - 1.0) <= 1e-5
    assert set(out["systematic"]) == {"source.fwhm", "source.depth"}
    total = out["systematic_total"]["p_sample"]
    assert math.isfinite(total) and total > 0.0
