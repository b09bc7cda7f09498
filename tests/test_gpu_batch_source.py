"""Sweeps under the laser-power source with per-point region monitors on the GPU (hf_batch_set_source, kb_source_load, hf_batch_set_monitors,
kb_monitor): the batch's source vectors bit for bit hf_set_source's, pulsed batched runs against the float64
restatement of tests/source_oracle.py and against single runs, linearity, the read-flux projection under a source, the absence of
side effects, kb_monitor bit for bit k_monitor (grouped launches included), the records of a run, the state rules and the driver.
Both small meshes, 20 steps at most."""
import copy
import functools
import math

import numpy as np
import pytest

import monitor_oracle as mo
import source_oracle as so
from conftest import build_case, load_cfg
from helpers import material_tables, reference_bcs

pytestmark = pytest.mark.gpu

FIELD_TOL_K = 1e-4     # against the restatement (tests/test_gpu_source.py)
SINGLE_TOL_K = 1e-5    # a column against its own hf_run (the batched parity tests of tests/test_gpu_parity.py)
FWHM = 1.4e-5
POWER = 0.2            # W, as the pulsed cases of tests/test_gpu_source.py: a rise of some tens of kelvin
KEPT_LINE_NAMES, KEPT_LINE_DEPTH, KEPT_LINE_POWER = ("p_coupler", "p_ins"), 5.0e-7, 0.5
NSTEPS = 20
NCOL = 16
CASES = {"with_diamond": "geballe_with_diamond", "no_diamond": "geballe_no_diamond"}
KINDS = {"shared": 0, "per_column": 1, "affine": 2}


@functools.lru_cache(maxsize=None)
def small(which):
    return build_case(CASES[which], 8.0)


def _dt(cfg):
    return float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])


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
    return HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, _dt(cfg), bcs, ic, **kw)


def _pulse(dt, nsteps=NSTEPS):
    return so.gaussian_pulse((np.arange(nsteps) + 1) * dt, 10 * dt, 8 * dt)


def _tags_z0(case, names):
    _, stack, mesh = case
    return [mesh.material_tags[n] for n in names], float(stack.by_name(names[0]).boundaries[0])


# 1. the source vectors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(CASES))
def test_batch_source_vectors_are_bit_for_bit_those_of_hf_set_source(hip, which):
    """nv = 4: columns 0 and 2 equal, column 1 with an infinite depth, column 3 with another width and depth."""
    case = small(which)
    _, _, mesh = case
    tags, z0 = _tags_z0(case, ("p_coupler", "p_ins"))
    fwhm = [FWHM, 0.9e-5, FWHM, 2.0e-5]
    depth = [2.0e-8, math.inf, 2.0e-8, 5.0e-7]
    bcs, ic = _bcs(case, True)
    prob = _problem(case, bcs, ic, precond=0)
    be = prob.backend
    try:
        be.batch_begin(4)
        be.batch_set_source(tags, fwhm, z0, depth)
        cols = [be.batch_get_source(j) for j in range(4)]
        be.batch_set_source(tags, fwhm, z0, depth)                        # the same batch again: the same bits
        assert all(np.array_equal(cols[j], be.batch_get_source(j)) for j in range(4))
        be.batch_end()
        for j in range(4):
            be.set_source(tags, fwhm[j], z0, depth[j])
            assert np.array_equal(cols[j], be.get_source()), j
        be.set_source(None)
    finally:
        prob.close()
    touched = np.zeros(len(mesh.coords), dtype=bool)
    touched[mesh.tris[np.isin(mesh.tags, tags)].ravel()] = True
    for j in range(4):
        assert np.all(cols[j][~touched] == 0.0) and not np.signbit(cols[j][~touched]).any() and np.all(cols[j][touched] > 0.0)
    assert np.array_equal(cols[0], cols[2]) and not np.array_equal(cols[0], cols[1]) and not np.array_equal(cols[0], cols[3])
    assert 100 < touched.sum() < len(touched)


# 2. pulsed runs against the restatement and against single runs -------------------------------------------------------------------------
def _column(j, keep_line, vary_k):
    """Column j of 16: power from half to twice the pulsed cases' (a factor 4 end to end), its own beam width and depth, and with
    per-column operators its own k of the sample."""
    base_depth, base_power = (KEPT_LINE_DEPTH, KEPT_LINE_POWER) if keep_line else (2.0e-8, POWER)
    return {"power": base_power * (0.5 + 1.5 * j / (NCOL - 1)), "fwhm": FWHM * (0.8 + 0.04 * j), "depth": base_depth * (1.0 + 0.25 * (j % 5)),
            "k": (3.3 + 0.07 * j) if vary_k else None}


def _columns(nv):
    return list(range(NCOL)) if nv == NCOL else [0, NCOL - 1]


@functools.lru_cache(maxsize=None)
def _restated(j, scheme, keep_line, vary_k):
    """(fields of column j's restated loop, its amplitudes, its peak rise by the source); computed once per combination."""
    case = small("with_diamond")
    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    col = _column(j, keep_line, vary_k)
    if vary_k:
        tk = dict(tk)
        tk[mesh.material_tags["p_sample"]] = col["k"]
    dt = _dt(cfg)
    bcs, ic = _bcs(case, keep_line)
    dofs, g_all = _boundary_values(bcs, dt, NSTEPS)
    tags, z0 = _tags_z0(case, KEPT_LINE_NAMES if keep_line else ("p_coupler",))
    F1, _ = so.source_vector(mesh.coords, mesh.tris, mesh.tags, tags, col["fwhm"], z0, col["depth"])
    amp = so.peak_density(col["power"], F1) * _pulse(dt)
    code = so.BDF2 if scheme == "bdf2" else so.BE
    args = (mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, np.full(len(mesh.coords), ic), g_all, F1)
    ref = so.sourced_fields(*args, amp, scheme=code)
    ref0 = so.sourced_fields(*args, np.zeros(NSTEPS), scheme=code)
    return ref, amp, float((ref - ref0).max())


@functools.lru_cache(maxsize=None)
def _single_runs(scheme, precond, keep_line, vary_k):
    """Every column's own hf_run (fields of all steps), one after the other on one context; computed once per combination."""
    case = small("with_diamond")
    _, _, mesh = case
    bcs, ic = _bcs(case, keep_line)
    prob = _problem(case, bcs, ic, precond=precond, scheme=scheme, amg_reuse=True)
    be = prob.backend
    out = []
    try:
        _, g_all = _boundary_values(bcs, prob.dt, NSTEPS)
        tags, z0 = _tags_z0(case, KEPT_LINE_NAMES if keep_line else ("p_coupler",))
        nodes = np.arange(prob.n, dtype=np.int32)
        for j in range(NCOL):
            col = _column(j, keep_line, vary_k)
            if vary_k:
                be.update_kappa([mesh.material_tags["p_sample"]], [col["k"]])
            be.set_source(tags, col["fwhm"], z0, col["depth"])
            be.set_source_amplitudes(_restated(j, scheme, keep_line, vary_k)[1])
            prob.set_state(ic)
            fields, _ = be.run(g_all, prob.rtol, 0.0, prob.max_it, nodes)
            out.append(fields)
    finally:
        prob.close()
    return out


PULSED = [(nv, kind, scheme, precond, False) for nv in (2, NCOL) for kind in sorted(KINDS) for scheme in ("backward_euler", "bdf2")
          for precond in (0, 1)] + [(nv, "shared", scheme, precond, True) for nv in (2, NCOL) for scheme in ("backward_euler", "bdf2")
                                    for precond in (0, 1)]


@pytest.mark.parametrize("nv, kind, scheme, precond, keep_line", PULSED)
def test_pulsed_batch_matches_the_restatement_and_single_runs(hip, nv, kind, scheme, precond, keep_line):
    case = small("with_diamond")
    _, _, mesh = case
    vary_k = kind != "shared"
    js = _columns(nv)
    cols = [_column(j, keep_line, vary_k) for j in js]
    refs = [_restated(j, scheme, keep_line, vary_k) for j in js]
    singles = _single_runs(scheme, precond, keep_line, vary_k)
    bcs, ic = _bcs(case, keep_line)
    prob = _problem(case, bcs, ic, precond=precond, scheme=scheme, amg_reuse=True)
    be = prob.backend
    tag_s = mesh.material_tags["p_sample"]
    try:
        _, g_one = _boundary_values(bcs, prob.dt, NSTEPS)
        tags, z0 = _tags_z0(case, KEPT_LINE_NAMES if keep_line else ("p_coupler",))
        if kind == "affine":
            ref_k = cols[nv // 2]["k"]
            be.update_kappa([tag_s], [ref_k])
            be.batch_begin(nv, per_column_operator=hip.BATCH_AFFINE)
            be.batch_set_affine([tag_s], [c["k"] - ref_k for c in cols])
        elif kind == "per_column":
            be.batch_begin(nv, per_column_operator=hip.BATCH_PER_COLUMN)
            for q, c in enumerate(cols):
                be.update_kappa([tag_s], [c["k"]])
                be.batch_load_column(q)
        else:
            be.batch_begin(nv)
        for q in range(nv):
            be.batch_set_state(q, np.full(prob.n, ic))
        be.batch_set_source(tags, [c["fwhm"] for c in cols], z0, [c["depth"] for c in cols])
        be.batch_set_source_amplitudes(np.stack([r[1] for r in refs], axis=1))
        fields, iters = be.batch_run(np.repeat(g_one[:, :, None], nv, axis=2), prob.rtol, 0.0, prob.max_it, np.arange(prob.n, dtype=np.int32))
        last = [be.batch_get_state(q) for q in range(nv)]
        be.batch_end()
    finally:
        prob.close()
    worst_ref = worst_one = 0.0
    for q, j in enumerate(js):
        assert np.array_equal(fields[-1, q], last[q])
        e_ref = float(np.abs(fields[:, q] - refs[q][0]).max())
        e_one = float(np.abs(fields[:, q] - singles[j]).max())
        worst_ref, worst_one = max(worst_ref, e_ref), max(worst_one, e_one)
        assert 10.0 <= refs[q][2] <= 500.0, (j, refs[q][2])             # tens of kelvin: a missing source cannot pass
    print(f"pulsed batch nv={nv} {kind} {scheme} precond={precond} keep_line={keep_line}: worst |dT| against the restatement "
          f"{worst_ref:.2e} K, against the single runs {worst_one:.2e} K, rises {refs[0][2]:.1f} .. {refs[-1][2]:.1f} K, "
          f"iterations {int(iters.sum())}")
    assert np.abs(fields[-1, 0] - fields[-1, nv - 1]).max() > 1.0       # the columns really differ
    assert worst_ref <= FIELD_TOL_K, f"{worst_ref:.3e} K"
    assert worst_one <= SINGLE_TOL_K, f"{worst_one:.3e} K"


# 3. linearity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_the_rise_of_a_column_is_linear_in_its_amplitude(hip, scheme):
    """Outer edges at ic_temp, one shared operator, two columns that differ only by p and 2 p: the rises differ by a factor 2 to
    1e-6 of the peak rise (the margin of two solves at the default rtol; tests/test_gpu_source.py)."""
    case = small("with_diamond")
    _, _, mesh = case
    tags, z0 = _tags_z0(case, ("p_coupler",))
    F1, _ = so.source_vector(mesh.coords, mesh.tris, mesh.tags, tags, FWHM, z0, 2.0e-8)
    bcs, ic = _bcs(case, False)
    prob = _problem(case, bcs, ic, precond=1, scheme=scheme)
    be = prob.backend
    try:
        _, g_one = _boundary_values(bcs, prob.dt, NSTEPS)
        amp = so.peak_density(POWER, F1) * _pulse(prob.dt)
        be.batch_begin(2)
        for q in range(2):
            be.batch_set_state(q, np.full(prob.n, ic))
        be.batch_set_source(tags, FWHM, z0, 2.0e-8)
        be.batch_set_source_amplitudes(np.stack([amp, 2.0 * amp], axis=1))
        fields, _ = be.batch_run(np.repeat(g_one[:, :, None], 2, axis=2), prob.rtol, 0.0, prob.max_it, np.arange(prob.n, dtype=np.int32))
        be.batch_end()
    finally:
        prob.close()
    rises = fields - ic
    peak = float(rises[:, 1].max())
    worst = float(np.abs(rises[:, 1] - 2.0 * rises[:, 0]).max())
    print(f"batched linearity {scheme}: peak rise {peak:.1f} K, worst |rise(2p) - 2 rise(p)| = {worst:.2e} K")
    assert peak >= 20.0
    assert worst <= 1e-6 * peak


# 4. the read-flux projection under a source -----------------------------------------------------------------------------------------------
def test_read_flux_of_a_batch_under_a_source_matches_the_single_runs(hip):
    from heatflow_amd.driver import FluxSampler

    case = small("no_diamond")
    _, _, mesh = case
    tags, z0 = _tags_z0(case, ("p_coupler",))
    nv, nsteps = 4, 12
    fwhm = [1.0e-5, FWHM, 1.8e-5, 2.4e-5]
    power = [0.1, 0.2, 0.3, 0.4]
    bcs, ic = _bcs(case, False)
    prob = _problem(case, bcs, ic, precond=1)
    be = prob.backend
    fnodes = FluxSampler(mesh.coords).nodes
    try:
        _, g_one = _boundary_values(bcs, prob.dt, nsteps)
        be.flux_setup()
        amps, singles = [], []
        for j in range(nv):
            be.set_source(tags, fwhm[j], z0, 2.0e-8)
            amps.append(so.peak_density(power[j], be.get_source()) * _pulse(prob.dt, nsteps))
            be.set_source_amplitudes(amps[-1])
            prob.set_state(ic)
            rows = []
            for k in range(nsteps):
                be.step(g_one[k], prob.rtol, 0.0, prob.max_it)
                be.flux_solve(prob.rtol, 5000, want_z=False)
                rows.append(be.flux_sample(fnodes, want_z=False)[1])
            singles.append(np.array(rows))
        be.set_source(None)
        be.batch_begin(nv)
        for j in range(nv):
            be.batch_set_state(j, np.full(prob.n, ic))
        be.batch_set_source(tags, fwhm, z0, 2.0e-8)
        be.batch_set_source_amplitudes(np.stack(amps, axis=1))
        _, _, grad = be.batch_run(np.repeat(g_one[:, :, None], nv, axis=2), prob.rtol, 0.0, prob.max_it, None, flux_nodes=fnodes,
                                  flux_components=2, flux_rtol=prob.rtol, flux_max_it=5000)
        # a run longer than the amplitudes left, through the flux entry point: refused by name, no step taken
        with pytest.raises(hip.HipError, match=r"hf_batch_run_flux: the source has 0 amplitudes left for 1 steps") as ei:
            be.batch_run(np.repeat(g_one[:1, :, None], nv, axis=2), prob.rtol, 0.0, prob.max_it, None, flux_nodes=fnodes)
        assert ei.value.code == hip.HF_ERR_STATE
        be.batch_end()
    finally:
        prob.close()
    for j in range(nv):
        scale = max(float(np.abs(singles[j]).max()), 1.0)
        err = float(np.abs(grad[:, 0, j] - singles[j]).max())
        print(f"read-flux under a source, column {j}: worst |d grad| = {err:.2e} K/m at a scale of {scale:.2e} K/m")
        assert scale > 1e5 and err <= 1e-4 * scale + 1e-3                # the bound of the batched sweep's gradient files
    assert np.abs(singles[0] - singles[3]).max() > 1e5


# 5. no side effect of the source --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
def test_a_source_that_was_removed_leaves_no_trace(hip, precond):
    case = small("with_diamond")
    tags, z0 = _tags_z0(case, ("p_coupler",))
    bcs, ic = _bcs(case, True)
    prob = _problem(case, bcs, ic, precond=precond)
    be = prob.backend
    out = []
    try:
        _, g_one = _boundary_values(bcs, prob.dt, 10)
        g_all = np.repeat(g_one[:, :, None], 2, axis=2)
        for with_source in (False, True):
            be.batch_begin(2)
            for q in range(2):
                be.batch_set_state(q, np.full(prob.n, ic))
            if with_source:
                be.batch_set_source(tags, [FWHM, 2.0e-5], z0, 2.0e-8)
                be.batch_set_source_amplitudes(np.full((10, 2), 1.0e15))
                be.batch_set_source(None)
            samples, iters = be.batch_run(g_all, prob.rtol, 0.0, prob.max_it, np.arange(prob.n, dtype=np.int32))
            out.append((samples, iters, be.batch_get_state(0), be.batch_get_state(1)))
            be.batch_end()
    finally:
        prob.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    assert out[0][0].max() > ic + 1.0                                    # the heated line drives these runs


# 6. kb_monitor bit for bit k_monitor ------------------------------------------------------------------------------------------------------------
def _thresholds(mesh):
    """Mixed: finite on the sample and the p-side insulation, +inf (None) on the two couplers, NaN (absent) elsewhere."""
    t = mesh.material_tags
    return {t["p_sample"]: 400.0, t["p_ins"]: 380.0, t["p_coupler"]: None, t["o_coupler"]: None}


def _varying_state(coords, seed=11):
    """Varies at every node: a smooth part plus noise, 300 .. 500 K (tests/test_gpu_monitors.py)."""
    rng = np.random.default_rng(seed)
    z, r = coords[:, 0], coords[:, 1]
    return 300.0 + 100.0 * rng.random(len(z)) + 50.0 * (1.0 + np.sin(z * 4.0e5)) * np.exp(-(r / 3.0e-5) ** 2)


def _check_against_restatement(rec, coords, tris, tags, u, thresholds, label):
    """rec [tab_len, 7] against the restatement of the state u: sums within (ne_t + 16) eps sum |term|, extremes and ids exact,
    unmonitored rows exact zeros (the check of tests/test_gpu_monitors.py)."""
    ref, scale, ne, _ = mo.per_tag(coords, tris, tags, u, thresholds, rec.shape[0])
    bound = mo.sum_bound(ne, scale)
    on = sorted(int(t) for t in thresholds)
    off = [t for t in range(rec.shape[0]) if t not in on]
    err = np.abs(rec[:, 4:] - ref[:, 4:])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))[on]
    print(f"{label}: worst error / bound  I0 I1 H = {ratio.max(axis=0)}")
    assert np.all(err[on] <= bound[on]), (label, ratio.max(axis=0))
    assert np.array_equal(rec[on, :4], ref[on, :4]), label
    assert np.all(rec[off] == 0.0) and not np.signbit(rec[off]).any()


def _batch_and_single_records(be, nv, states):
    """(batch_monitor_now() of the columns `states`, [monitor_now() after set_state of each]) on an assembled context with monitors."""
    be.batch_begin(nv)
    for j, u in enumerate(states):
        be.batch_set_state(j, u)
    be.batch_set_monitors(True)
    rec = be.batch_monitor_now()
    assert be.batch_monitor_count() == 0 and np.array_equal(rec, be.batch_monitor_now())       # nothing is recorded; the same bits again
    be.batch_end()
    singles = []
    for u in states:
        be.set_state(u)
        singles.append(be.monitor_now())
    return rec, singles


def _assert_every_branch(coords, tris, tags, states, th):
    for u in states:
        assert len(np.unique(u)) == len(u)
        branches = mo.per_tag(coords, tris, tags, u, th)[3]
        for t, v in th.items():
            if v is not None and math.isfinite(v) and v < 1.0e3:
                assert np.all(branches[t] > 0), (t, branches[t])        # triangles with 0, 1, 2 and 3 nodes above: every branch of the cut


@pytest.mark.parametrize("nv", [2, 4, 8, 16])
@pytest.mark.parametrize("which", sorted(CASES))
def test_kb_monitor_is_bit_for_bit_k_monitor_on_the_small_meshes(hip, which, nv):
    case = small(which)
    _, _, mesh = case
    th = _thresholds(mesh)
    states = [_varying_state(mesh.coords, 11 + j) for j in range(nv)]
    _assert_every_branch(mesh.coords, mesh.tris, mesh.tags, states, th)
    bcs, ic = _bcs(case, True)
    prob = _problem(case, bcs, ic, precond=0)
    be = prob.backend
    try:
        be.set_monitors(th)
        rec, singles = _batch_and_single_records(be, nv, states)
    finally:
        prob.close()
    assert rec.shape == (nv, int(mesh.tags.max()) + 1, 7)
    for j in range(nv):
        assert np.array_equal(rec[j], singles[j]), j                     # node ids and all
    assert not np.array_equal(rec[0], rec[nv - 1])
    _check_against_restatement(rec[nv - 1], mesh.coords, mesh.tris, mesh.tags, states[nv - 1], th, f"kb_monitor {which} nv={nv} column {nv - 1}")


@functools.lru_cache(maxsize=None)
def _grid_mesh(stripes):
    """The 70 688-triangle grid of tests/test_gpu_monitors.py (277 chunks of 256 on 272 workgroups), in `stripes` stripes of z."""
    nz = nr = 188
    z, r = np.meshgrid(np.linspace(0.0, 4.0e-5, nz + 1), np.linspace(0.0, 2.0e-5, nr + 1), indexing="ij")
    coords = np.stack([z.ravel(), r.ravel()], axis=1)
    idx = np.arange((nz + 1) * (nr + 1)).reshape(nz + 1, nr + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.stack([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)], axis=1).reshape(-1, 3).astype(np.int32)
    zc = coords[tris][:, :, 0].mean(axis=1)
    tags = (1 + np.minimum((zc / 4.0e-5 * stripes).astype(np.int32), stripes - 1)).astype(np.int32)
    assert len(tris) == 70688 and (len(tris) + 255) // 256 == 277
    return coords, tris, tags


def _grid_context(hip, coords, tris, tags):
    """An assembled context on the grid (a batch needs one): unit-order coefficients, the z = 0 edge held, Jacobi."""
    be = hip.HeatflowHIP()
    be.set_mesh(coords, tris, tags)
    present = sorted(int(t) for t in np.unique(tags))
    be.set_materials(present, [10.0] * len(present), [2.76e6] * len(present))
    be.set_dirichlet(np.nonzero(coords[:, 0] == 0.0)[0].astype(np.int32))
    be.set_precond(0)
    be.assemble(2.0e-9, hip.ASM_ROW_GATHER)
    be.set_state(np.full(len(coords), 300.0))
    return be


@pytest.mark.parametrize("nv", [2, 4, 8, 16])
def test_kb_monitor_on_a_mesh_with_more_chunks_than_workgroups(hip, nv):
    coords, tris, tags = _grid_mesh(5)
    th = {1: 420.0, 2: None, 4: 390.0, 5: 1.0e4}
    states = [_varying_state(coords, 11 + j) for j in range(nv)]
    _assert_every_branch(coords, tris, tags, states, th)
    with _grid_context(hip, coords, tris, tags) as be:
        be.set_monitors(th)
        rec, singles = _batch_and_single_records(be, nv, states)
    for j in range(nv):
        assert np.array_equal(rec[j], singles[j]), j
        assert rec[j, 5, 6] == 0.0 and np.all(rec[j, 3] == 0.0) and rec[j, 1, 6] > 0.0
    _check_against_restatement(rec[0], coords, tris, tags, states[0], th, f"kb_monitor grid nv={nv} column 0")


def test_kb_monitor_in_grouped_launches_with_forty_monitored_tags(hip):
    """40 stripes, all monitored, 16 columns: the per-wave accumulators of the six per-column fields are 4 x 40 x 16 x 40 B = 100 KB,
    more than one workgroup may ask for, so the columns go in two launches of eight."""
    nv = 16
    coords, tris, tags = _grid_mesh(40)
    # thresholds that follow the smooth part of the states from stripe to stripe, so that every stripe is cut; every seventh: no hot part
    th = {t: (None if t % 7 == 0 else round(350.0 + 41.0 * (1.0 + math.sin((t - 0.5) * 1.0e-6 * 4.0e5)), 1)) for t in range(1, 41)}
    states = [_varying_state(coords, 11 + j) for j in range(nv)]
    _assert_every_branch(coords, tris, tags, states, th)
    with _grid_context(hip, coords, tris, tags) as be:
        be.set_monitors(th)
        rec, singles = _batch_and_single_records(be, nv, states)
    for j in range(nv):
        assert np.array_equal(rec[j], singles[j]), j
    _check_against_restatement(rec[nv - 1], coords, tris, tags, states[nv - 1], th, "kb_monitor grid 40 tags column 15")
    assert all(rec[0, t, 4] > 0.0 and (rec[0, t, 6] > 0.0) == (th[t] is not None) for t in range(1, 41))


# 7. the records of a run ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond, scheme", [(0, "backward_euler"), (1, "bdf2")])
def test_every_step_of_a_batched_run_leaves_the_record_of_its_state(hip, precond, scheme):
    case = small("with_diamond")
    _, _, mesh = case
    th = _thresholds(mesh)
    tags, z0 = _tags_z0(case, ("p_coupler",))
    nv = 4
    bcs, ic = _bcs(case, True)
    prob = _problem(case, bcs, ic, precond=precond, scheme=scheme)
    be = prob.backend
    nodes = np.array([0, prob.n // 2, prob.n - 1], dtype=np.int32)
    try:
        _, g_one = _boundary_values(bcs, prob.dt, NSTEPS)
        g_all = np.repeat(g_one[:, :, None], nv, axis=2)
        be.set_monitors(th)
        be.step(g_one[0])                                                 # the context's own record: untouched by what follows
        own = be.get_monitors()
        assert be.monitor_count() == 1
        F1 = None
        runs = []
        for monitors in (True, False):
            be.batch_begin(nv)
            for q in range(nv):
                be.batch_set_state(q, np.full(prob.n, ic))
            be.batch_set_source(tags, [FWHM, 1.0e-5, FWHM, 2.0e-5], z0, [2.0e-8, 2.0e-8, math.inf, 4.0e-8])
            if F1 is None:
                F1 = [be.batch_get_source(q) for q in range(nv)]
            be.batch_set_source_amplitudes(np.stack([so.peak_density(POWER * (1 + q), F1[q]) * _pulse(prob.dt) for q in range(nv)], axis=1))
            if monitors:
                be.batch_set_monitors(True)
            parts, snaps = [], {}
            for a, b in ((0, 1), (1, 7), (7, NSTEPS)):                   # stopped after steps 1, 7 and 20
                parts.append(be.batch_run(g_all[a:b], prob.rtol, 0.0, prob.max_it, nodes))
                snaps[b] = [be.batch_get_state(q) for q in range(nv)]
                if monitors:
                    assert be.batch_monitor_count() == b
            if monitors:
                hist = be.batch_get_monitors()
                assert np.array_equal(be.batch_get_monitors(6, 2), hist[6:8])
                assert np.array_equal(be.batch_monitor_now(), hist[-1]) and be.batch_monitor_count() == NSTEPS
                with pytest.raises(ValueError, match=r"hf_batch_get_monitors: records \[19, 21\) outside the 20 records kept"):
                    be.batch_get_monitors(19, 2)
            runs.append((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), snaps))
            be.batch_end()
        assert be.monitor_count() == 1 and np.array_equal(be.get_monitors(), own)
        assert hist.shape == (NSTEPS, nv, int(mesh.tags.max()) + 1, 7)
        for k, states in runs[0][2].items():
            for q in range(nv):
                be.set_state(states[q])
                assert np.array_equal(hist[k - 1, q], be.monitor_now()), (k, q)
        _check_against_restatement(hist[-1, 1], mesh.coords, mesh.tris, mesh.tags, runs[0][2][NSTEPS][1], th, "batch record, step 20, column 1")
    finally:
        prob.close()
    # the switch changes nothing else: samples, iteration counts and states bit for bit
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        for q in range(nv):
            assert np.array_equal(runs[0][2][k][q], runs[1][2][k][q])
    tc = mesh.material_tags["p_coupler"]
    assert hist[:, :, tc, 0].max() > ic + 10.0 and not np.array_equal(hist[-1, 0], hist[-1, 1])
    assert np.array_equal(hist[:, :, :, 4], np.broadcast_to(hist[0, 0, :, 4], hist[:, :, :, 4].shape))       # I0 is the mesh's: the same bits


# 8. state rules ------------------------------------------------------------------------------------------------------------------------------------
def _state_error(hip, fn, pattern):
    with pytest.raises(hip.HipError, match=pattern) as ei:
        fn()
    assert ei.value.code == hip.HF_ERR_STATE


def test_error_returns_and_state_rules(hip):
    case = small("with_diamond")
    _, _, mesh = case
    tags, z0 = _tags_z0(case, ("p_coupler",))
    tag = tags[0]
    bcs, ic = _bcs(case, True)
    prob = _problem(case, bcs, ic, precond=0)
    be = prob.backend
    try:
        g = prob.bc_values(prob.dt)
        g2 = np.stack([g, g], axis=1)
        # without a batch
        for fn, name in ((lambda: be.batch_set_source(tags, FWHM, z0), "hf_batch_set_source"), (lambda: be.batch_get_source(0), "hf_batch_get_source"),
                         (lambda: be.batch_set_source_amplitudes(np.ones((1, 2))), "hf_batch_set_source_amplitudes"),
                         (lambda: be.batch_set_monitors(True), "hf_batch_set_monitors"), (be.batch_monitor_now, "hf_batch_monitor_now"),
                         (be.batch_monitor_count, "hf_batch_monitor_count"), (lambda: be.batch_get_monitors(0, 0), "hf_batch_get_monitors")):
            _state_error(hip, fn, rf"{name}: no batch is open")
        be.batch_begin(2)
        # without monitors on the context, and before the switch
        _state_error(hip, lambda: be.batch_set_monitors(True), "hf_batch_set_monitors: no monitors set")
        _state_error(hip, be.batch_monitor_now, "hf_batch_monitor_now: the batch's monitors are off")
        _state_error(hip, lambda: be.batch_get_monitors(0, 0), "hf_batch_get_monitors: the batch's monitors are off")
        assert be.batch_monitor_count() == 0
        be.batch_set_monitors(False)
        # without a source
        _state_error(hip, lambda: be.batch_get_source(0), "hf_batch_get_source: no source set")
        _state_error(hip, lambda: be.batch_set_source_amplitudes(np.ones((1, 2))), "hf_batch_set_source_amplitudes: no source set")
        # hf_set_source's checks, per column
        unused = int(mesh.tags.max()) + 5
        for args, pat in ((([unused], FWHM, z0), rf"hf_batch_set_source: tag {unused} is not a cell tag"),
                          (([tag, tag], FWHM, z0), rf"hf_batch_set_source: tag {tag} is listed twice"),
                          (([tag], [FWHM, 0.0], z0), "hf_batch_set_source: fwhm must be positive"),
                          (([tag], [math.inf, FWHM], z0), "hf_batch_set_source: fwhm must be positive and finite"),
                          (([tag], FWHM, math.nan), "hf_batch_set_source: z0 must be finite"),
                          (([tag], FWHM, z0, [2.0e-8, 0.0]), "hf_batch_set_source: depth must be positive"),
                          (([tag], FWHM, z0, [math.nan, 2.0e-8]), "hf_batch_set_source: depth must be positive")):
            with pytest.raises(ValueError, match=pat):
                be.batch_set_source(*args)
        with pytest.raises(ValueError, match="batch_set_source: fwhm must be a scalar or 2 values"):       # a bad column count
            be.batch_set_source([tag], [FWHM] * 3, z0)
        _state_error(hip, lambda: be.batch_get_source(0), "no source set")                 # a refused call sets nothing
        be.batch_set_source([tag], FWHM, z0, [math.inf, 2.0e-8])                           # +inf is a depth
        with pytest.raises(ValueError, match="hf_batch_get_source: bad column"):
            be.batch_get_source(2)
        with pytest.raises(ValueError, match="hf_batch_set_source_amplitudes: the amplitude of step 1, column 0 is not finite"):
            be.batch_set_source_amplitudes([[1.0, 1.0], [math.inf, 1.0]])
        with pytest.raises(ValueError, match=r"batch_set_source_amplitudes: p must be \(n_steps, 2\)"):
            be.batch_set_source_amplitudes(np.ones((2, 3)))
        # a run beyond the table, before any launch: the states do not move
        for q in range(2):
            be.batch_set_state(q, np.full(prob.n, ic))
        be.batch_set_source_amplitudes(np.zeros((2, 2)))
        _state_error(hip, lambda: be.batch_run(np.stack([g2, g2, g2])), r"hf_batch_run: the source has 2 amplitudes left for 3 steps")
        assert np.array_equal(be.batch_get_state(0), np.full(prob.n, ic))
        be.batch_run(np.stack([g2, g2]))
        _state_error(hip, lambda: be.batch_run(np.stack([g2])), r"hf_batch_run: the source has 0 amplitudes left for 1 steps")
        be.batch_set_source_amplitudes(None)                                                  # an empty table: amplitude 0, any number of steps
        be.batch_run(np.stack([g2, g2, g2]))
        # the context's own source stays out of a batch, and the batch's dies with it
        _state_error(hip, lambda: be.set_source([tag], FWHM, z0), "hf_set_source: a batch is open")
        be.batch_end()
        _state_error(hip, lambda: be.batch_get_source(0), "hf_batch_get_source: no batch is open")
        be.batch_begin(2)
        _state_error(hip, lambda: be.batch_get_source(0), "hf_batch_get_source: no source set")
        be.batch_end()
        be.set_source([tag], FWHM, z0)
        _state_error(hip, lambda: be.batch_begin(2), "hf_batch_begin: a source is set")
        be.set_source(None)
        # records are gone after batch_end; the context's count never moved
        be.set_monitors({tag: 301.0})
        be.batch_begin(2)
        for q in range(2):
            be.batch_set_state(q, np.full(prob.n, ic))
        be.batch_set_monitors(True)
        be.batch_run(np.stack([g2, g2]))
        assert be.batch_monitor_count() == 2
        be.batch_set_monitors(True)                                                            # the switch again drops the records
        assert be.batch_monitor_count() == 0
        be.batch_run(np.stack([g2]))
        assert be.batch_monitor_count() == 1
        be.batch_set_monitors(False)
        assert be.batch_monitor_count() == 0
        _state_error(hip, be.batch_monitor_now, "the batch's monitors are off")
        be.batch_set_monitors(True)
        be.batch_run(np.stack([g2]))
        be.batch_end()
        assert be.monitor_count() == 0
        be.batch_begin(2)
        assert be.batch_monitor_count() == 0
        _state_error(hip, lambda: be.batch_get_monitors(0, 0), "the batch's monitors are off")
        be.batch_end()
    finally:
        prob.close()


# 9. the driver -----------------------------------------------------------------------------------------------------------------------------------------
def test_run_batch_over_the_beam_width_with_monitors_against_single_runs(hip):
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small("with_diamond")
    base = copy.deepcopy(load_cfg("geballe_with_diamond_source"))
    base["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in base["mats"].items()}
    base["timing"] = dict(base["timing"], num_steps=NSTEPS, t_final=NSTEPS * 7.5e-8, sweep_monitors=True)
    base["heating"]["source"].update(pulse={"t0": 7.5e-7, "fwhm": 6.0e-7}, sweeps=True)
    del base["heating"]["source"]["fwhm"]                                 # the beam follows heating.fwhm
    base["monitors"] = {"sample": {"material": "p_sample", "above": 301.0}, "coupler": {"material": ["p_coupler", "o_coupler"]}}
    cfgs = []
    for f in (8.0e-6, 1.32e-5, 2.0e-5, 3.0e-5):
        c = copy.deepcopy(base)
        c["heating"]["fwhm"] = f
        cfgs.append(c)
    stacks = [build_stack(c) for c in cfgs]
    wp = get_watcher_points(cfgs[0])
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags)
    try:
        res = s.run_batch(cfgs, stacks, wp)
        singles = [s.run(c, st, wp) for c, st in zip(cfgs, stacks)]
    finally:
        s.close()
    peaks = []
    for j, (r, one) in enumerate(zip(res, singles)):
        for nm in one["watchers"]:
            assert np.abs(r["watchers"][nm] - one["watchers"][nm]).max() <= SINGLE_TOL_K, (j, nm)
        assert list(r["monitors"]) == list(one["monitors"]) == ["sample", "coupler"]
        for region, fields in one["monitors"].items():
            assert set(r["monitors"][region]) == set(fields)
            for field in ("z_max", "r_max", "z_min", "r_min"):           # the peak nodes are the same
                assert np.array_equal(r["monitors"][region][field], fields[field]), (j, region, field)
            for field in ("volume", "T_mean", "energy", "hot_volume"):  # sums: 1e-9 relative
                if field in fields:
                    a, b = r["monitors"][region][field], fields[field]
                    assert np.all(np.abs(a - b) <= 1e-9 * np.abs(b)), (j, region, field, float(np.abs(a - b).max()))
            assert np.abs(r["monitors"][region]["T_max"] - fields["T_max"]).max() <= SINGLE_TOL_K
        peaks.append(float(r["monitors"]["coupler"]["T_max"].max()))
    print("coupler peak by beam fwhm:", peaks)
    assert peaks[0] > peaks[1] > peaks[2] > peaks[3] > 301.0             # the same power through a narrower beam
