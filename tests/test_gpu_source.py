"""Laser-power heating on the GPU (hf_set_source, hf_set_source_amplitudes) against the float64 restatement of
tests/source_oracle.py: the source vector F1 entry by entry, its zero rows and its reproducibility, all-ones amplitudes against
the existing load path bit for bit, 20 pulsed steps field by field (both small meshes, both preconditioners, both schemes,
every start-vector kind, with and without the heated line), a pulse on top of a hold load, linearity in the amplitude, the
Picard right-hand side under tables, the error and state rules, and the energy balance at 1.04 M DOF."""
import functools
import math

import numpy as np
import pytest

import source_oracle as so
from conftest import build_case
from helpers import material_tables, reference_bcs
from heatflow_amd.solver import DEFAULT_RTOL
from rhoc_T_oracle import einstein_tables
from test_gpu_kappa_T import _ins_tables
from test_gpu_steady import STEADY_RTOL, hold_load_restated, restated_steady, stiffness, two_line_steady

pytestmark = pytest.mark.gpu

FIELD_TOL_K = 1e-4
# 4 ln2 r^2 / fwhm^2 <= 100 on both small meshes (r <= 8e-5 m gives 90.6), so rounding the argument of exp costs at most
# 100 * 2^-53 = 1.2e-14 relative in s
FWHM = 1.4e-5
POWER = 0.2            # W: a peak rise of 58 K (with diamonds) and 85 K (without) in the restatement, three edges at ic_temp
# With the heated line kept, the 62 nm coupler is one element thick and every node of its outer face is a Dirichlet row, so a
# source in the coupler alone moves the free nodes by 0.05 K at 0.2 W in the restatement.  Those runs therefore absorb in the
# coupler and the insulation behind it over 0.5 um, at 0.5 W: 43 K (with diamonds) and 50 K (without) on top of the line's
# own heating, with 22 % of the load falling on Dirichlet rows, where it must change nothing.
KEPT_LINE_NAMES, KEPT_LINE_DEPTH, KEPT_LINE_POWER = ("p_coupler", "p_ins"), 5.0e-7, 0.5
NSTEPS = 20
CASES = {"with_diamond": "geballe_with_diamond", "no_diamond": "geballe_no_diamond"}


@functools.lru_cache(maxsize=None)
def small(which):
    return build_case(CASES[which], 8.0)


def _dt(cfg):
    return float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])


def _source(case, names=("p_coupler",), depth=math.inf, fwhm=FWHM):
    _, stack, mesh = case
    return {"tags": [mesh.material_tags[n] for n in names], "fwhm": fwhm, "z0": float(stack.by_name(names[0]).boundaries[0]),
            "depth": depth}


def _restated_vector(case, source):
    _, _, mesh = case
    return so.source_vector(mesh.coords, mesh.tris, mesh.tags, source["tags"], source["fwhm"], source["z0"], source["depth"])


def _bcs(case, keep_line):
    cfg, stack, mesh = case
    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    return (bcs if keep_line else bcs[:3]), ic


def _boundary_values(bcs, dt, nsteps):
    """(dofs, g_all) as HeatProblem.run tabulates them: every condition at t = 0, then the heated line (if any) per step."""
    from heatflow_amd.bc import gather_bc_values, gather_plan, merge_bcs

    dofs, owner, pos = merge_bcs(bcs)
    for bc in bcs:
        bc.update(0.0)
    plan = gather_plan(len(bcs), owner, pos)
    g_all = []
    for k in range(nsteps):
        for bc in bcs[3:]:
            bc.update((k + 1) * dt)
        g_all.append(gather_bc_values(bcs, owner, pos, plan).copy())
    return np.asarray(dofs, dtype=np.int64), np.array(g_all)


def _problem(case, bcs, ic, **kw):
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    kw.setdefault("dt", _dt(cfg))
    dt = kw.pop("dt")
    return HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, bcs, ic, **kw)


def _pulse(dt, nsteps=NSTEPS):
    """A Gaussian pulse whose peak (step 10) falls inside the run."""
    return so.gaussian_pulse((np.arange(nsteps) + 1) * dt, 10 * dt, 8 * dt)


def _run_fields(prob, nsteps, amp=None):
    _, fields, iters = prob.run(nsteps, watcher_nodes=np.arange(prob.n, dtype=np.int32), time_varying=prob.bcs[3:],
                                **({} if amp is None else {"source_amplitude": amp}))
    return fields, iters


# 1. F1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which, names, depth", [
    ("with_diamond", ("p_coupler",), math.inf), ("with_diamond", ("p_coupler",), 2.0e-8),
    ("with_diamond", ("p_coupler", "p_ins"), math.inf), ("with_diamond", ("p_coupler", "p_ins"), 5.0e-7),
    ("no_diamond", ("p_coupler",), 2.0e-8), ("no_diamond", ("o_coupler", "p_sample"), math.inf)])
def test_source_vector_matches_the_restatement(hip, which, names, depth):
    """|F1_i - ref_i| <= 1e-13 sum_j |M1_ij| s_j: a row sums at most 32 entries of a few roundings each, and s itself carries
    the rounded argument of exp (at most 1.2e-14 relative at this fwhm) and the exp routine's last bits."""
    case = small(which)
    _, _, mesh = case
    source = _source(case, names, depth)
    ref, scale = _restated_vector(case, source)
    with hip.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_source(source["tags"], source["fwhm"], source["z0"], source["depth"])
        F = be.get_source()
    live = scale > 0.0
    ratio = float((np.abs(F - ref)[live] / scale[live]).max())
    print(f"F1 {which} {names} depth={depth}: worst |F1 - ref| / sum |M1| s = {ratio:.2e}, sum F1 = {F.sum():.6e}")
    assert np.all(np.abs(F - ref) <= 1e-13 * scale), ratio
    assert live.sum() > 100 and np.all(F[~live] == 0.0)


def test_rows_without_an_absorbing_triangle_are_exactly_zero_and_two_calls_give_the_same_bits(hip):
    case = small("with_diamond")
    _, _, mesh = case
    source = _source(case, ("p_coupler",), 2.0e-8)
    touched = np.zeros(len(mesh.coords), dtype=bool)
    touched[mesh.tris[np.isin(mesh.tags, source["tags"])].ravel()] = True
    out = []
    for _ in range(2):
        with hip.HeatflowHIP() as be:
            be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
            be.set_source(source["tags"], source["fwhm"], source["z0"], source["depth"])
            first = be.get_source()
            be.set_source(source["tags"], source["fwhm"], source["z0"], source["depth"])      # the same context again
            assert np.array_equal(first, be.get_source())
            out.append(first)
    assert np.array_equal(out[0], out[1])                                                      # and a fresh context
    assert np.all(out[0][~touched] == 0.0) and not np.signbit(out[0][~touched]).any()
    assert np.all(out[0][touched] > 0.0) and touched.sum() < len(touched) // 4


# 2. all-ones amplitudes are the existing load path ----------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_all_ones_amplitudes_are_bitwise_the_load_path(hip, scheme, precond):
    """source_amplitude all ones against set_load(source_vector()) through the path of before: w = dt' * 1 is dt' itself and
    the vector is the same.  At 1 W/m^3 the source moves nothing a double can hold, so the comparison is repeated at 2^50 W/m^3
    (a rise of 2.8 K over the 8 steps in the restatement, outer edges only), where both dt' * p and p * F1 are exact scalings
    and the bits must still agree."""
    case = small("with_diamond")
    source = _source(case, ("p_coupler",), 2.0e-8)
    nsteps = 8
    last = {}
    for p in (1.0, 2.0 ** 50):
        fields = []
        for through_load in (False, True):
            bcs, ic = _bcs(case, False)
            prob = _problem(case, bcs, ic, precond=precond, scheme=scheme, source=source)
            try:
                if through_load:
                    F1 = prob.source_vector()
                    prob.backend.set_source(None)
                    prob.source = None                  # (the problem no longer hands amplitudes over)
                    prob.set_load(F1 * p)
                    fields.append(_run_fields(prob, nsteps)[0])
                else:
                    fields.append(_run_fields(prob, nsteps, np.full(nsteps, p))[0])
            finally:
                prob.close()
        assert np.array_equal(fields[0], fields[1]), f"p = {p}"
        last[p] = fields[0]
    assert np.abs(last[2.0 ** 50] - last[1.0]).max() > 1.0


# 3. 20 pulsed steps against the restatement -------------------------------------------------------------------------------------
def _pulsed_source(case, keep_line):
    """(source, absorbed power in W) of the pulsed runs."""
    if keep_line:
        return _source(case, KEPT_LINE_NAMES, KEPT_LINE_DEPTH), KEPT_LINE_POWER
    return _source(case, ("p_coupler",), 2.0e-8), POWER


@functools.lru_cache(maxsize=None)
def _reference(which, scheme, keep_line):
    """(fields with the pulse, fields without any source, amplitudes) of the restated loop; computed once per combination."""
    case = small(which)
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    dt = _dt(cfg)
    bcs, ic = _bcs(case, keep_line)
    dofs, g_all = _boundary_values(bcs, dt, NSTEPS)
    source, power = _pulsed_source(case, keep_line)
    F1, _ = _restated_vector(case, source)
    amp = so.peak_density(power, F1) * _pulse(dt)
    code = so.BDF2 if scheme == "bdf2" else so.BE
    args = (mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, np.full(len(mesh.coords), ic), g_all, F1)
    return so.sourced_fields(*args, amp, scheme=code), so.sourced_fields(*args, np.zeros(NSTEPS), scheme=code), amp


@pytest.mark.parametrize("keep_line", [False, True])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("which", ["with_diamond", "no_diamond"])
def test_pulsed_run_matches_the_restatement_at_every_step(hip, which, precond, scheme, kind, keep_line):
    case = small(which)
    ref, ref0, amp = _reference(which, scheme, keep_line)
    bcs, ic = _bcs(case, keep_line)
    prob = _problem(case, bcs, ic, precond=precond, scheme=scheme, source=_pulsed_source(case, keep_line)[0])
    try:
        prob.backend.set_start_vector(kind)
        fields, iters = _run_fields(prob, NSTEPS, amp)
    finally:
        prob.close()
    worst = float(np.abs(fields - ref).max())
    rise = float((ref - ref0).max())
    print(f"pulsed {which} precond={precond} {scheme} kind={kind} keep_line={keep_line}: worst |dT| = {worst:.2e} K, "
          f"peak rise by the source {rise:.1f} K, iterations {int(np.sum(iters))}")
    assert 10.0 <= rise <= 500.0                       # tens of kelvin: a missing source cannot pass
    assert worst <= FIELD_TOL_K, f"{worst:.3e} K"


# 4. a pulse on top of a hold load ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
def test_source_on_top_of_a_hold_load(hip, precond):
    from heatflow_amd.bc import gather_bc_values, merge_bcs

    case = small("with_diamond")
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    sb = two_line_steady(case)
    source = _source(case, ("p_coupler",), 2.0e-8)
    prob = _problem(case, sb[:3], float(cfg["heating"]["ic_temp"]), precond=precond, source=source, max_it=400000)
    try:
        prob.rtol = STEADY_RTOL
        u_ss, _, _ = prob.solve_steady(sb)
        prob.rtol = DEFAULT_RTOL
        prob.hold_load()
        # amplitude 0: the held state stays, as without a source
        fields, _ = _run_fields(prob, 10)
        drift = float(np.abs(fields - u_ss).max())
        print(f"hold + source precond={precond}: drift at amplitude 0 = {drift:.2e} K")
        assert drift <= 1e-5, f"{drift:.3e} K"
        # the pulse from the held state against the restatement
        prob.set_state(u_ss)
        dt = prob.dt
        F1, _ = _restated_vector(case, source)
        amp = so.peak_density(POWER, F1) * _pulse(dt)
        fields, _ = _run_fields(prob, NSTEPS, amp)
        K, _ = stiffness(case)
        sd, so_, sp_ = merge_bcs(sb)
        u_ref = restated_steady(K, sd, gather_bc_values(sb, so_, sp_))
        B = np.asarray(prob.bc_dofs, dtype=np.int64)
        F0 = hold_load_restated(K, u_ref, B)
        g = np.full(len(B), float(cfg["heating"]["ic_temp"]))
        ref = so.sourced_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, B, u_ref, [g] * NSTEPS, F1, amp, load=F0)
        worst = float(np.abs(fields - ref).max())
        rise = float((ref - u_ref).max())
        print(f"hold + source precond={precond}: worst |dT| = {worst:.2e} K, peak rise {rise:.1f} K")
        assert rise >= 10.0 and worst <= FIELD_TOL_K, f"{worst:.3e} K"
    finally:
        prob.close()


# 5. linearity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_the_rise_is_linear_in_the_amplitude(hip, scheme):
    """Outer edges at ic_temp, no heated line: amplitudes p and 2 p give rises that differ by a factor 2 to 1e-6 of the peak
    rise - the margin of two solves at the default rtol, not of rounding."""
    case = small("with_diamond")
    source = _source(case, ("p_coupler",), 2.0e-8)
    F1, _ = _restated_vector(case, source)
    rises = []
    for factor in (1.0, 2.0):
        bcs, ic = _bcs(case, False)
        prob = _problem(case, bcs, ic, precond=1, scheme=scheme, source=source)
        try:
            amp = factor * so.peak_density(POWER, F1) * _pulse(prob.dt)
            rises.append(_run_fields(prob, NSTEPS, amp)[0] - ic)
        finally:
            prob.close()
    peak = float(rises[1].max())
    worst = float(np.abs(rises[1] - 2.0 * rises[0]).max())
    print(f"linearity {scheme}: peak rise {peak:.1f} K, worst |rise(2p) - 2 rise(p)| = {worst:.2e} K")
    assert peak >= 20.0 and worst <= 1e-6 * peak


# 6. tables: the Picard right-hand side ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [("k",), ("c",), ("k", "c")])
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_sourced_run_under_tables_matches_the_restatement(hip, scheme, kinds):
    case = small("with_diamond")
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    ktab = _ins_tables(stack, mesh, tk) if "k" in kinds else {}
    ctab = einstein_tables(trc, [mesh.material_tags[m] for m in ("p_ins", "o_ins", "g_ins", "p_coupler")]) if "c" in kinds else {}
    source = _source(case, ("p_coupler",), 2.0e-8)
    nsteps = 10
    bcs, ic = _bcs(case, False)
    dt = _dt(cfg)
    dofs, g_all = _boundary_values(bcs, dt, nsteps)
    F1, _ = _restated_vector(case, source)
    amp = 4.0 * so.peak_density(POWER, F1) * so.gaussian_pulse((np.arange(nsteps) + 1) * dt, 5 * dt, 4 * dt)
    code = so.BDF2 if scheme == "bdf2" else so.BE
    args = (mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, np.full(len(mesh.coords), ic), g_all, F1, amp)
    ref = so.sourced_fields(*args, scheme=code, kappa_tables=ktab, rhoc_tables=ctab, picard=2)
    lin = so.sourced_fields(*args, scheme=code)
    prob = _problem(case, bcs, ic, precond=1, scheme=scheme, source=source, picard=2,
                    **({"kappa_tables": ktab} if ktab else {}), **({"rhoc_tables": ctab} if ctab else {}))
    try:
        fields, _ = _run_fields(prob, nsteps, amp)
    finally:
        prob.close()
    worst = float(np.abs(fields - ref).max())
    print(f"tables {kinds} {scheme}: worst |dT| = {worst:.2e} K, peak rise {ref.max() - ic:.1f} K, "
          f"tables move the answer by {np.abs(ref - lin).max():.2e} K")
    assert ref.max() - ic >= 10.0
    assert np.abs(ref - lin).max() > 100 * FIELD_TOL_K           # the tables matter, so the sweeps' right-hand side is exercised
    assert worst <= FIELD_TOL_K, f"{worst:.3e} K"


# 7. errors and state rules -----------------------------------------------------------------------------------------------------
def _state_error(hip, fn, pattern):
    with pytest.raises(hip.HipError, match=pattern) as ei:
        fn()
    assert ei.value.code == hip.HF_ERR_STATE


def test_error_returns_and_state_rules(hip):
    case = small("with_diamond")
    _, stack, mesh = case
    tag = mesh.material_tags["p_coupler"]
    z0 = float(stack.by_name("p_coupler").boundaries[0])
    with hip.HeatflowHIP() as be:
        _state_error(hip, lambda: be.set_source([tag], FWHM, z0), "hf_set_source before hf_set_mesh")
    bcs, ic = _bcs(case, True)
    prob = _problem(case, bcs, ic, precond=0)
    be = prob.backend
    try:
        _state_error(hip, be.get_source, "hf_get_source: no source set")
        _state_error(hip, lambda: be.set_source_amplitudes([1.0]), "hf_set_source_amplitudes: no source set")
        unused = int(mesh.tags.max()) + 5
        for args, pat in ((([unused], FWHM, z0), rf"hf_set_source: tag {unused} is not a cell tag"),
                          (([0], FWHM, z0), "hf_set_source: tag 0 is not a cell tag"),
                          (([-1], FWHM, z0), "hf_set_source: tag -1 is not a cell tag"),
                          (([tag, tag], FWHM, z0), rf"hf_set_source: tag {tag} is listed twice"),
                          (([tag], 0.0, z0), "hf_set_source: fwhm must be positive"),
                          (([tag], math.inf, z0), "hf_set_source: fwhm must be positive and finite"),
                          (([tag], math.nan, z0), "hf_set_source: fwhm must be positive"),
                          (([tag], FWHM, math.nan), "hf_set_source: z0 must be finite"),
                          (([tag], FWHM, z0, 0.0), "hf_set_source: depth must be positive"),
                          (([tag], FWHM, z0, -1e-8), "hf_set_source: depth must be positive"),
                          (([tag], FWHM, z0, math.nan), "hf_set_source: depth must be positive")):
            with pytest.raises(ValueError, match=pat):
                be.set_source(*args)
        _state_error(hip, be.get_source, "no source set")                 # a refused call sets nothing
        be.set_source([tag], FWHM, z0, math.inf)                          # +inf is a depth
        with pytest.raises(ValueError, match="hf_set_source_amplitudes: amplitude 1 is not finite"):
            be.set_source_amplitudes([1.0, math.inf])
        # a step beyond the list, before any launch: the state does not move
        be.set_source_amplitudes([0.0, 0.0])
        u0 = be.get_state()
        g = prob.bc_values(prob.dt)
        _state_error(hip, lambda: be.run(np.stack([g, g, g])), r"hf_run: the source has 2 amplitudes left for 3 steps")
        assert np.array_equal(be.get_state(), u0)
        be.run(np.stack([g, g]))
        _state_error(hip, lambda: be.step(g), r"hf_step: the source has 0 amplitudes left for 1 steps")
        be.set_source_amplitudes([])                                       # an empty list: amplitude 0, any number of steps
        be.step(g)
        # the batched loop and the tangents refuse a source, and open again once it is cleared
        _state_error(hip, lambda: be.batch_begin(2), "hf_batch_begin: a source is set")
        _state_error(hip, lambda: be.tangent_setup(1, {tag: 0}), "hf_tangent_setup: a source is set")
        _state_error(hip, lambda: be.tangent_setup_dir(1, r={tag: 0}), "hf_tangent_setup_dir: a source is set")
        be.set_source(None)
        be.batch_begin(2)
        _state_error(hip, lambda: be.set_source([tag], FWHM, z0), "hf_set_source: a batch is open")
        be.batch_end()
        be.tangent_setup_dir(1, r={tag: 0})
        be.tangent_setup(1, {tag: 0})
        be.set_source([tag], FWHM, z0)
        _state_error(hip, lambda: be.run_tangent(np.stack([g])), "hf_run_tangent: a source is set")
        be.set_source(None)
        be.run_tangent(np.stack([g]))
        # the source survives the materials, an assembly and a conductivity update; a new mesh clears it
        be.set_source([tag], FWHM, z0, 2.0e-8)
        F1 = be.get_source()
        tk, trc = material_tables(stack, mesh)
        prob.set_materials({t: 2.0 * k for t, k in tk.items()}, trc)
        be.update_kappa([tag], [100.0])
        assert np.array_equal(be.get_source(), F1)
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        _state_error(hip, be.get_source, "no source set")
    finally:
        prob.close()


def test_a_mesh_without_row_gather_lists_refuses_a_source(hip):
    """More than 64 distinct cell tags: the row-gather lists do not exist for such a mesh, and k_source_load runs on them."""
    nz, nr = 7, 8
    z, r = np.meshgrid(np.arange(nz) * 1.0e-6, np.arange(nr) * 1.0e-6, indexing="ij")
    coords = np.column_stack([z.ravel(), r.ravel()])
    q = (np.arange(nz - 1)[:, None] * nr + np.arange(nr - 1)[None, :]).ravel()
    tris = np.concatenate([np.column_stack([q, q + nr, q + nr + 1]), np.column_stack([q, q + nr + 1, q + 1])]).astype(np.int32)
    tags = np.arange(1, len(tris) + 1, dtype=np.int32)
    assert len(tags) > 64
    with hip.HeatflowHIP() as be:
        be.set_mesh(coords, tris, tags)
        with pytest.raises(ValueError, match="hf_set_source: the source's load is formed by the row-gather kernel only"):
            be.set_source([1], FWHM, 0.0)
        _state_error(hip, be.get_source, "no source set")


@pytest.mark.parametrize("precond", [0, 1])
def test_cleared_source_is_bitwise_the_run_without_one(hip, precond):
    case = small("with_diamond")
    source = _source(case, ("p_coupler",), 2.0e-8)
    runs = []
    for had_source in (True, False):
        bcs, ic = _bcs(case, True)
        prob = _problem(case, bcs, ic, precond=precond)
        try:
            if had_source:
                prob.backend.set_source(source["tags"], source["fwhm"], source["z0"], source["depth"])
                prob.backend.set_source_amplitudes([1.0e20] * 3)
                prob.backend.set_source(None)
            runs.append(_run_fields(prob, 6)[0])
        finally:
            prob.close()
    assert np.array_equal(runs[0], runs[1])
    assert np.abs(runs[1][-1] - runs[1][0]).max() > 0.0


# 8. 1.04 M DOF --------------------------------------------------------------------------------------------------------------------
C3_DT = 1.0e-9        # s
C3_POWER = 0.1        # W: a peak rise of 32 K in the restatement on the small mesh


def test_energy_balance_at_one_million_dof_with_multigrid(hip):
    """20 pulsed steps at C3 with the multigrid preconditioner: no Jacobi fallback, and sum_i (M u)_i grows by
    dt sum_k p_k sum_i F1_i to 1e-6 relative.  Summing the free rows of the step equation cancels the stiffness
    (sum_i K_ij = 0) up to the rows next to a Dirichlet row, so the identity holds while no heat has reached those rows.
    The choice that guarantees it: the p-side coupler absorbs, the beam is 4 um wide, and the step is 1 ns, so that 20 steps
    (20 ns) spread the heat over a fraction of a micrometre while the nearest Dirichlet row's neighbours lie 3.2 um away
    (across the p-side insulator) - on the small mesh, where a coarse element spans more of that distance per hop than on the
    fine one, the restatement's rise at every neighbour of a Dirichlet node stays below 1e-9 K (asserted here first)."""
    import time

    # the choice, checked in the restatement on the small mesh
    case_s = small("with_diamond")
    cfg, stack_s, mesh_s = case_s
    tk, trc = material_tables(stack_s, mesh_s)
    bcs_s, ic = _bcs(case_s, False)
    dofs_s, g_s = _boundary_values(bcs_s, C3_DT, NSTEPS)
    src_s = _source(case_s, ("p_coupler",), 2.0e-8, fwhm=4.0e-6)
    F1_s, _ = _restated_vector(case_s, src_s)
    amp_s = so.peak_density(C3_POWER, F1_s) * _pulse(C3_DT)
    ref = so.sourced_fields(mesh_s.coords, mesh_s.tris, mesh_s.tags, tk, trc, C3_DT, dofs_s, np.full(len(mesh_s.coords), ic),
                            g_s, F1_s, amp_s)
    M1 = so.absorbing_mass(mesh_s.coords, mesh_s.tris, mesh_s.tags, set(int(t) for t in mesh_s.tags))
    near = np.unique(M1[dofs_s].indices)
    rise_near = float(np.abs(ref[:, near] - ic).max())
    print(f"small mesh: peak rise {ref.max() - ic:.1f} K, largest rise next to a Dirichlet node {rise_near:.2e} K")
    assert rise_near <= 1e-9 and ref.max() - ic >= 10.0

    case = build_case("geballe_with_diamond", 0.43)
    _, stack, mesh = case
    assert len(mesh.coords) > 1_000_000
    bcs, ic = _bcs(case, False)
    source = _source(case, ("p_coupler",), 2.0e-8, fwhm=4.0e-6)
    # rtol: the stopping rule is relative to ||D^-1 b|| ~ 300 K on 1e6 rows while the balance is about a rise on a few thousand
    # rows, so the default 1e-10 leaves the sum a margin of about 1e-7 relative per step; 1e-12 takes the solver out of the bound
    prob = _problem(case, bcs, ic, precond=1, source=source, dt=C3_DT, rtol=1e-12)
    try:
        be = prob.backend
        F1 = prob.source_vector()
        sumF1 = math.fsum(F1)
        amp = C3_POWER / (2.0 * math.pi * sumF1) * _pulse(C3_DT)
        u0 = be.get_state()
        t0 = time.perf_counter()
        _, _, iters = prob.run(NSTEPS, source_amplitude=amp)
        wall = time.perf_counter() - t0
        gpu_ms = be.last_gpu_ms()
        u = be.get_state()
        got = math.fsum(be.spmv(u - u0, which=1))           # sum_i (M (u - u0))_i: the difference first, so nothing cancels
        info = be.amg_info()
    finally:
        prob.close()
    want = C3_DT * math.fsum(amp) * sumF1
    print(f"C3 source: n = {len(mesh.coords)}, iterations per step {list(map(int, iters))}, {gpu_ms / NSTEPS:.3f} ms per step on the "
          f"GPU ({1e3 * wall / NSTEPS:.3f} ms wall), peak rise {u.max() - ic:.1f} K, sum(M u) grew by {got:.9e} (expected {want:.9e}, "
          f"relative difference {abs(got - want) / want:.2e}), Jacobi fallbacks {info['jacobi_fallbacks']}")
    assert info["jacobi_fallbacks"] == 0
    assert u.max() - ic >= 10.0
    assert abs(got - want) <= 1e-6 * want
