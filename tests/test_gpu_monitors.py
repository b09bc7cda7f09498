"""Region monitors on the GPU (hf_set_monitors, k_monitor) against the float64 restatement of tests/monitor_oracle.py:
monitor_now with mixed thresholds and every branch of the cut, the edge rules, analytic linear fields, reproducibility, the
records of hf_step / hf_run / hf_run_tangent, the absence of side effects, the energy identity, the error and state rules and
the driver.  Both small meshes, 20 steps at most."""
import copy
import csv
import functools
import math
import re

import numpy as np
import pytest

import monitor_oracle as mo
import source_oracle as so
from conftest import build_case, load_cfg
from helpers import material_tables, reference_bcs
from rhoc_T_oracle import einstein_tables
from test_gpu_kappa_T import _ins_tables

pytestmark = pytest.mark.gpu

CASES = {"with_diamond": "geballe_with_diamond", "no_diamond": "geballe_no_diamond"}
MATS = ("p_sample", "p_ins", "p_coupler")
REL = 1e-12
NSTEPS = 20
FWHM = 1.4e-5


@functools.lru_cache(maxsize=None)
def small(which):
    return build_case(CASES[which], 8.0)


def _thresholds(mesh):
    """Mixed: finite on the sample and the p-side insulation, +inf (None) on the two couplers, NaN (absent) elsewhere."""
    t = mesh.material_tags
    return {t["p_sample"]: 400.0, t["p_ins"]: 380.0, t["p_coupler"]: None, t["o_coupler"]: None}


def _varying_state(mesh, seed=11):
    """Varies at every node: a smooth part plus noise, 300 .. 500 K."""
    rng = np.random.default_rng(seed)
    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    return 300.0 + 100.0 * rng.random(len(z)) + 50.0 * (1.0 + np.sin(z * 4.0e5)) * np.exp(-(r / 3.0e-5) ** 2)


def _check_against_restatement(rec, mesh, u, thresholds, label):
    """rec [tab_len, 7] against the restatement of the state u: sums within (ne_t + 16) eps sum |term|, extremes and ids exact,
    unmonitored rows exact zeros.  Returns the worst ratio error / bound of I0, I1, H."""
    ref, scale, ne, _ = mo.per_tag(mesh.coords, mesh.tris, mesh.tags, u, thresholds, rec.shape[0])
    bound = mo.sum_bound(ne, scale)
    on = sorted(int(t) for t in thresholds)
    off = [t for t in range(rec.shape[0]) if t not in on]
    err = np.abs(rec[:, 4:] - ref[:, 4:])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))[on]
    worst = ratio.max(axis=0)
    print(f"{label}: worst error / bound  I0 {worst[0]:.3f}  I1 {worst[1]:.3f}  H {worst[2]:.3f}  "
          f"(relative to sum |term|: {np.nanmax(np.where(scale[on] > 0, err[on] / np.where(scale[on] > 0, scale[on], 1.0), 0.0)):.2e})")
    assert np.all(err[on] <= bound[on]), (label, worst)
    assert np.array_equal(rec[on, :4], ref[on, :4]), (label, rec[on, :4], ref[on, :4])
    assert np.all(rec[off] == 0.0) and not np.signbit(rec[off]).any()
    return worst


# 1. monitor_now against the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(CASES))
def test_monitor_now_matches_the_restatement(hip, which):
    _, _, mesh = small(which)
    th = _thresholds(mesh)
    u = _varying_state(mesh)
    assert len(np.unique(u)) == len(u)
    _, _, _, branches = mo.per_tag(mesh.coords, mesh.tris, mesh.tags, u, th)
    for t, v in th.items():
        if v is not None:
            assert np.all(branches[t] > 0), (t, branches[t])           # triangles with 0, 1, 2 and 3 nodes above: every branch of the cut
    with hip.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_state(u)
        be.set_monitors(th)
        rec = be.monitor_now()
        assert be.monitor_count() == 0                                  # nothing is recorded
    assert rec.shape == (int(mesh.tags.max()) + 1, 7)
    _check_against_restatement(rec, mesh, u, th, f"monitor_now {which}")
    for t, v in th.items():
        assert (rec[t, 6] == 0.0) == (v is None) and rec[t, 4] > 0.0


def test_a_mesh_with_more_chunks_than_a_workgroup_takes_at_once(hip):
    """70 688 triangles are 277 chunks of 256: the grid is 272 workgroups (a multiple of 8, the per-XCD schedule), so some
    workgroups add a second chunk to their accumulators and some chunks hold two tags - the paths neither small mesh reaches."""
    nz = nr = 188
    z, r = np.meshgrid(np.linspace(0.0, 4.0e-5, nz + 1), np.linspace(0.0, 2.0e-5, nr + 1), indexing="ij")
    coords = np.stack([z.ravel(), r.ravel()], axis=1)
    idx = np.arange((nz + 1) * (nr + 1)).reshape(nz + 1, nr + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.stack([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)], axis=1).reshape(-1, 3).astype(np.int32)
    zc = coords[tris][:, :, 0].mean(axis=1)
    tags = (1 + np.minimum((zc / 4.0e-5 * 5).astype(np.int32), 4)).astype(np.int32)         # five stripes in z: tags 1..5
    assert len(tris) == 70688 and (len(tris) + 255) // 256 == 277

    class G:
        pass
    mesh = G()
    mesh.coords, mesh.tris, mesh.tags = coords, tris, tags
    th = {1: 420.0, 2: None, 4: 390.0, 5: 1.0e4}
    u = _varying_state(mesh, 31)
    _, _, _, branches = mo.per_tag(coords, tris, tags, u, th)
    assert np.all(branches[1] > 0) and np.all(branches[4] > 0) and branches[5, 0] == np.count_nonzero(tags == 5)
    with hip.HeatflowHIP() as be:
        be.set_mesh(coords, tris, tags)
        be.set_state(u)
        be.set_monitors(th)
        rec = be.monitor_now()
        assert np.array_equal(rec, be.monitor_now())
    _check_against_restatement(rec, mesh, u, th, "monitor_now grid 70688")
    assert rec[5, 6] == 0.0 and rec[3, 4] == 0.0


# 2. edge rules ----------------------------------------------------------------------------------------------------------------------------
def test_plateau_exact_threshold_and_one_ulp_above(hip):
    _, _, mesh = small("with_diamond")
    tag, other = mesh.material_tags["p_sample"], mesh.material_tags["p_ins"]
    nodes = np.unique(mesh.tris[mesh.tags == tag])
    rng = np.random.default_rng(3)
    u = 300.0 + 50.0 * rng.random(len(mesh.coords))
    plateau = np.sort(rng.choice(nodes, 9, replace=False))
    u[plateau] = 400.0
    low = np.sort(rng.choice(np.setdiff1d(nodes, plateau), 5, replace=False))
    u[low] = 250.0
    theta = 1234.5
    with hip.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_monitors({tag: theta, other: 320.0})
        be.set_state(u)
        rec = be.monitor_now()
        assert rec[tag, 0] == 400.0 and rec[tag, 1] == plateau[0]       # a plateau of equal maxima: the smallest id
        assert rec[tag, 2] == 250.0 and rec[tag, 3] == low[0]
        u[nodes] = theta                                                 # the whole tag held at exactly theta
        be.set_state(u)
        rec = be.monitor_now()
        assert rec[tag, 6] == 0.0 and not np.signbit(rec[tag, 6]) and rec[tag, 0] == theta and rec[tag, 1] == nodes.min()
        assert rec[other, 6] > 0.0
        u[nodes] = np.nextafter(theta, math.inf)                         # one ulp above: the whole tag
        be.set_state(u)
        rec = be.monitor_now()
    ref, scale, ne, _ = mo.per_tag(mesh.coords, mesh.tris, mesh.tags, u, {tag: theta, other: 320.0})
    bound = mo.sum_bound(ne, scale)[tag, 0]
    print(f"one ulp above theta: |H - I0| = {abs(rec[tag, 6] - rec[tag, 4]):.2e}, bound {bound:.2e}")
    assert abs(rec[tag, 6] - rec[tag, 4]) <= bound and abs(rec[tag, 6] - ref[tag, 4]) <= bound


# 3. analytic fields ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(CASES))
def test_linear_fields_against_analytic_values(hip, which):
    _, stack, mesh = small(which)
    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    with hip.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_monitors({mesh.material_tags[n]: 300.0 for n in MATS})
        for name in MATS:
            tag = mesh.material_tags[name]
            z0, z1, r0, r1 = (float(v) for v in stack.by_name(name).boundaries[:4])
            vol = math.pi * (r1 * r1 - r0 * r0) * (z1 - z0)
            zs, cz = z0 + 0.37 * (z1 - z0), 1.0e8
            be.set_state(300.0 + cz * (z - zs))
            rec = be.monitor_now()
            hot, mean = math.pi * (r1 * r1 - r0 * r0) * (z1 - zs), 300.0 + cz * (0.5 * (z0 + z1) - zs)
            e = (abs(2 * math.pi * rec[tag, 4] - vol) / vol, abs(2 * math.pi * rec[tag, 6] - hot) / hot, abs(rec[tag, 5] / rec[tag, 4] - mean) / abs(mean))
            rstar, cr = r0 + 0.41 * (r1 - r0), 1.0e7
            be.set_state(300.0 - cr * (r - rstar))
            rec = be.monitor_now()
            hot = math.pi * (rstar * rstar - r0 * r0) * (z1 - z0)
            mean = 300.0 - cr * ((2.0 / 3.0) * (r1 ** 3 - r0 ** 3) / (r1 * r1 - r0 * r0) - rstar)
            e += (abs(2 * math.pi * rec[tag, 6] - hot) / hot, abs(rec[tag, 5] / rec[tag, 4] - mean) / abs(mean))
            print(f"analytic {which} {name}: volume {e[0]:.1e}, hot (z) {e[1]:.1e}, mean (z) {e[2]:.1e}, hot (r) {e[3]:.1e}, mean (r) {e[4]:.1e}")
            assert max(e) <= REL, (name, e)


# 4. reproducibility -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_two_contexts_give_the_same_bits(hip):
    _, _, mesh = small("no_diamond")
    th = _thresholds(mesh)
    u = _varying_state(mesh, 23)
    out = []
    for _ in range(2):
        with hip.HeatflowHIP() as be:
            be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
            be.set_state(u)
            be.set_monitors(th)
            first = be.monitor_now()
            assert np.array_equal(first, be.monitor_now())
            be.set_monitors(th)                                          # the table again
            assert np.array_equal(first, be.monitor_now())
            out.append(first)
    assert np.array_equal(out[0], out[1])


# 5. records ---------------------------------------------------------------------------------------------------------------------------------
def _dt(cfg):
    return float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])


def _source(case, power_names=("p_coupler",)):
    _, stack, mesh = case
    return {"tags": [mesh.material_tags[n] for n in power_names], "fwhm": FWHM, "z0": float(stack.by_name(power_names[0]).boundaries[0]),
            "depth": 2.0e-8}


def _problem(case, kind, precond=1, scheme="backward_euler", monitors=True, **kw):
    """kind: "dirichlet" (the heated line drives), "source" (three edges, absorbed power), "tables" (k(T) and cv(T), picard = 2)."""
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    if kind == "source":
        bcs = bcs[:3]
        kw["source"] = _source(case)
    if kind == "tables":
        kw.update(kappa_tables=_ins_tables(stack, mesh, tk), picard=2,
                  rhoc_tables=einstein_tables(trc, [mesh.material_tags[m] for m in ("p_ins", "o_ins", "g_ins", "p_coupler")]))
    prob = HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, _dt(cfg), bcs, ic, precond=precond, scheme=scheme, **kw)
    if monitors:
        prob.backend.set_monitors(_thresholds(mesh))
    return prob


def _amplitudes(prob, nsteps, power):
    F1 = prob.source_vector()
    return so.peak_density(power, F1) * so.gaussian_pulse((np.arange(nsteps) + 1) * prob.dt, 10 * prob.dt, 8 * prob.dt)


RECORD_CASES = [("with_diamond", "dirichlet", 0, "backward_euler"), ("with_diamond", "dirichlet", 1, "bdf2"),
                ("no_diamond", "dirichlet", 1, "backward_euler"), ("no_diamond", "dirichlet", 0, "bdf2"),
                ("with_diamond", "source", 1, "backward_euler"), ("no_diamond", "source", 0, "bdf2"),
                ("with_diamond", "tables", 1, "backward_euler")]


@pytest.mark.parametrize("which, kind, precond, scheme", RECORD_CASES)
def test_every_step_of_hf_step_leaves_the_record_of_its_state(hip, which, kind, precond, scheme):
    case = small(which)
    _, _, mesh = case
    th = _thresholds(mesh)
    prob = _problem(case, kind, precond, scheme)
    be = prob.backend
    nsteps = 6
    try:
        amp = _amplitudes(prob, nsteps, 0.5) if kind == "source" else None
        for bc in prob.bcs:
            bc.update(0.0)
        worst = np.zeros(3)
        for k in range(nsteps):
            prob.step((k + 1) * prob.dt, only=prob.bcs[3:], **({"source_amplitude": float(amp[k])} if amp is not None else {}))
            assert be.monitor_count() == k + 1
            rec = be.get_monitors(k, 1)[0]
            assert np.array_equal(rec, be.monitor_now()), k            # bit for bit the current state's
            worst = np.maximum(worst, _check_against_restatement(rec, mesh, be.get_state(), th, f"hf_step {which} {kind} step {k}"))
        hist = be.get_monitors()
        assert hist.shape == (nsteps, int(mesh.tags.max()) + 1, 7) and np.array_equal(hist[-1], rec)
    finally:
        prob.close()
    print(f"hf_step {which} {kind} precond={precond} {scheme}: worst error / bound over {nsteps} steps {worst}")


@pytest.mark.parametrize("which, kind, precond, scheme", RECORD_CASES)
def test_hf_run_of_20_steps_leaves_20_records(hip, which, kind, precond, scheme):
    case = small(which)
    _, _, mesh = case
    th = _thresholds(mesh)
    prob = _problem(case, kind, precond, scheme)
    be = prob.backend
    try:
        amp = _amplitudes(prob, NSTEPS, 0.5) if kind == "source" else None
        _, fields, _ = prob.run(NSTEPS, watcher_nodes=np.arange(prob.n, dtype=np.int32), time_varying=prob.bcs[3:],
                                **({"source_amplitude": amp} if amp is not None else {}))
        assert be.monitor_count() == NSTEPS
        hist = be.get_monitors()
        assert np.array_equal(hist[-1], be.monitor_now()) and np.array_equal(fields[-1], be.get_state())
        worst = np.zeros(3)
        for k in range(NSTEPS):                                             # every record is its own step's
            worst = np.maximum(worst, _check_against_restatement(hist[k], mesh, fields[k], th, f"hf_run {which} {kind} step {k}"))
        print(f"hf_run {which} {kind} precond={precond} {scheme}: worst error / bound over {NSTEPS} steps {worst}")
        tc = mesh.material_tags["p_coupler"]
        assert hist[:, tc, 0].max() > 301.0                                 # the run heats
        assert np.array_equal(hist[:, :, 4], np.broadcast_to(hist[0, :, 4], hist[:, :, 4].shape))    # I0 is the mesh's: the same bits
        assert np.array_equal(be.get_monitors(7, 3), hist[7:10])
    finally:
        prob.close()


@pytest.mark.parametrize("which, precond", [("with_diamond", 1), ("no_diamond", 0)])
def test_hf_run_tangent_records_the_primal_state(hip, which, precond):
    case = small(which)
    _, _, mesh = case
    th = _thresholds(mesh)
    prob = _problem(case, "dirichlet", precond)
    be = prob.backend
    nodes = np.arange(prob.n, dtype=np.int32)
    try:
        _, fields, _, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=[[mesh.material_tags["p_sample"]]], time_varying=prob.bcs[3:])
        assert be.monitor_count() == NSTEPS
        hist = be.get_monitors()
        assert np.array_equal(hist[-1], be.monitor_now()) and np.array_equal(fields[-1], be.get_state())
        for k in range(NSTEPS):                                             # the primal state of every step
            _check_against_restatement(hist[k], mesh, fields[k], th, f"hf_run_tangent {which} precond={precond} step {k}")
        assert np.abs(prob.tangent(0)).max() > 0.0
    finally:
        prob.close()


# 6. no side effects ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("tangent", [False, True])
def test_monitors_change_nothing_else(hip, precond, tangent):
    case = small("with_diamond")
    _, _, mesh = case
    runs = []
    for monitors in (False, True):
        prob = _problem(case, "dirichlet", precond, monitors=monitors)
        nodes = np.arange(prob.n, dtype=np.int32)
        try:
            if tangent:
                _, s, ts, it, tit = prob.run_tangent(NSTEPS, nodes, conductivity=[[mesh.material_tags["p_sample"]]], time_varying=prob.bcs[3:])
                runs.append((s, ts, it, tit, prob.state(), prob.tangent(0)))
            else:
                _, s, it = prob.run(NSTEPS, watcher_nodes=nodes, time_varying=prob.bcs[3:])
                runs.append((s, it, prob.state()))
            assert prob.backend.monitor_count() == (NSTEPS if monitors else 0)
        finally:
            prob.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert np.abs(runs[0][0][-1] - runs[0][0][0]).max() > 1.0


# 7. the energy identity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(CASES))
def test_energy_of_all_tags_is_the_mass_weighted_rise(hip, which):
    """2 pi sum_t rho_c_t (I1_t - T_ref I0_t) over all tags after 20 sourced steps against 2 pi sum_i (M (u - T_ref))_i with M from
    hf_get_csr, within (3 ne + 16) eps sum_ij |M_ij| |u_j - T_ref|.  The left side is a difference of the cell's whole heat content
    at 300 K, so its resolution is an ulp of that, whatever the rise, while the bound scales with the rise: the pulse is 2 W (a
    rise of some hundred kelvin, about 1e-6 J deposited) so that the bound stands above that floor."""
    import scipy.sparse as sp

    case = small(which)
    _, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    prob = _problem(case, "source", 1, monitors=False)
    be = prob.backend
    try:
        be.set_monitors({t: None for t in trc})
        T_ref = 300.0
        prob.run(NSTEPS, source_amplitude=_amplitudes(prob, NSTEPS, 2.0))
        rec = be.get_monitors()[-1]
        u = be.get_state()
        rowptr, colidx, _, Mv = be.get_csr()
    finally:
        prob.close()
    M = sp.csr_matrix((Mv, colidx, rowptr), shape=(len(u), len(u)))
    du = u - T_ref
    want = 2.0 * math.pi * math.fsum(M @ du)
    bound = 2.0 * math.pi * (3 * len(mesh.tris) + 16) * mo.EPS * math.fsum(abs(M) @ np.abs(du))
    got = mo.energy(rec, trc, T_ref)
    content = 2.0 * math.pi * sum(trc[t] * rec[t, 5] for t in trc)
    print(f"energy {which}: {got:.12e} J against {want:.12e} J, difference {abs(got - want):.2e}, bound {bound:.2e} "
          f"(ratio {abs(got - want) / bound:.3f}); peak rise {u.max() - T_ref:.1f} K, heat content {content:.3e} J")
    assert u.max() - T_ref >= 50.0 and want > 1e-7
    assert abs(got - want) <= bound


# 8. errors and lifetime -------------------------------------------------------------------------------------------------------------------------
def _state_error(hip, fn, pattern):
    with pytest.raises(hip.HipError, match=pattern) as ei:
        fn()
    assert ei.value.code == hip.HF_ERR_STATE


def test_error_returns_and_lifetime(hip):
    case = small("with_diamond")
    _, stack, mesh = case
    tag = mesh.material_tags["p_sample"]
    tab_len = int(mesh.tags.max()) + 1
    with hip.HeatflowHIP() as be:
        be.tab_len = tab_len
        _state_error(hip, lambda: be.set_monitors({tag: 1.0}), "hf_set_monitors before hf_set_mesh")
        _state_error(hip, be.monitor_now, "hf_monitor_now before hf_set_mesh")
        _state_error(hip, be.monitor_count, "hf_monitor_count before hf_set_mesh")
        _state_error(hip, lambda: be.get_monitors(0, 0), "hf_get_monitors before hf_set_mesh")
        _state_error(hip, be.clear_monitor_records, "hf_monitor_clear before hf_set_mesh")
    prob = _problem(case, "dirichlet", 0, monitors=False)
    be = prob.backend
    try:
        _state_error(hip, be.monitor_now, r"hf_monitor_now: no monitors set")
        _state_error(hip, lambda: be.get_monitors(0, 0), r"hf_get_monitors: no monitors set")
        assert be.monitor_count() == 0
        unused = tab_len + 4
        for th, pat in (({unused: 1.0}, rf"hf_set_monitors: tag {unused} is not a cell tag of the mesh"),
                        ({0: None}, "hf_set_monitors: tag 0 is not a cell tag of the mesh"),
                        ({tag: -math.inf}, rf"hf_set_monitors: the threshold of tag {tag} is -inf")):
            with pytest.raises(ValueError, match=pat):
                be.set_monitors(th)
        with pytest.raises(ValueError, match=r"set_monitors: tag -1 is not a cell tag"):
            be.set_monitors({-1: 1.0})
        with pytest.raises(ValueError, match=rf"set_monitors: the threshold of tag {tag} is NaN"):
            be.set_monitors({tag: math.nan})
        _state_error(hip, be.monitor_now, "no monitors set")                # a refused call sets nothing
        be.set_monitors({tag: 350.0})
        g = prob.bc_values(prob.dt)
        be.run(np.stack([g, g, g]))
        assert be.monitor_count() == 3
        for first, count, pat in ((0, 4, r"hf_get_monitors: records \[0, 4\) outside the 3 records kept"),
                                  (-1, 1, r"hf_get_monitors: records \[-1, 0\) outside"), (3, 1, r"records \[3, 4\) outside"),
                                  (1, -1, r"records \[1, 0\) outside")):
            with pytest.raises(ValueError, match=pat):
                be.get_monitors(first, count)
        assert be.get_monitors(3, 0).shape == (0, tab_len, 7)
        for fn, args, pat in ((be._lib.hf_monitor_now, (None,), "hf_monitor_now: null pointer"),
                              (be._lib.hf_monitor_count, (None,), "hf_monitor_count: null pointer"),
                              (be._lib.hf_get_monitors, (0, 1, None), r"hf_get_monitors: null pointer for records \[0, 1\)")):
            assert fn(be._ctx, *args) == hip.HF_ERR_ARG and re.search(pat, be._lib.hf_last_error(be._ctx).decode())
        # a step that fails leaves no record
        with pytest.raises(hip.NotConverged):
            be.step(g + 50.0, prob.rtol, 0.0, 1)
        assert be.monitor_count() == 3
        # the monitors survive the materials, an assembly, a new state, the table, source and steady calls
        last = be.get_monitors(2, 1)[0]
        tk, trc = material_tables(stack, mesh)
        prob.set_materials({t: 2.0 * k for t, k in tk.items()}, trc)
        be.set_source([mesh.material_tags["p_coupler"]], FWHM, 0.0)
        be.set_source(None)
        be.set_state(np.full(prob.n, 300.0))
        be.steady_setup(prob.bc_dofs, 0)
        be.steady_solve(g)                                                  # a steady solve records nothing; monitor_now serves it
        assert be.monitor_count() == 3 and np.array_equal(be.get_monitors(2, 1)[0], last)
        now = be.monitor_now()
        assert now[tag, 0] >= 300.0 and now[tag, 4] == last[tag, 4]
        be.set_kappa_tables(_ins_tables(stack, mesh, tk), 1)
        be.set_kappa_tables({})
        be.set_state(np.full(prob.n, 300.0))
        be.assemble(prob.dt, 3)
        be.step(g)
        assert be.monitor_count() == 4
        # hf_monitor_clear keeps the table
        be.clear_monitor_records()
        assert be.monitor_count() == 0
        with pytest.raises(ValueError, match=r"records \[0, 1\) outside the 0 records kept"):
            be.get_monitors(0, 1)
        be.step(g)
        assert be.monitor_count() == 1 and be.get_monitors()[0, tag, 4] == last[tag, 4]
        # an open batch refuses; the batched loop records nothing
        be.batch_begin(2)
        for fn, name in ((lambda: be.set_monitors({tag: 1.0}), "hf_set_monitors"), (be.monitor_now, "hf_monitor_now"),
                         (be.monitor_count, "hf_monitor_count"), (lambda: be.get_monitors(0, 1), "hf_get_monitors"),
                         (be.clear_monitor_records, "hf_monitor_clear")):
            _state_error(hip, fn, rf"{name}: a batch is open")
        be.batch_set_state(0, np.full(prob.n, 300.0))
        be.batch_set_state(1, np.full(prob.n, 300.0))
        be.batch_run(np.stack([np.stack([g, g], axis=1)] * 2))
        be.batch_end()
        assert be.monitor_count() == 1
        # an all-NaN table, an empty one and NULL remove the monitors; so does a new mesh
        be.set_monitors({})
        _state_error(hip, be.monitor_now, "no monitors set")
        be.set_monitors({tag: None})
        nan = np.full(tab_len, np.nan)
        import ctypes as C
        assert be._lib.hf_set_monitors(be._ctx, tab_len, nan.ctypes.data_as(C.POINTER(C.c_double))) == hip.HF_OK
        _state_error(hip, be.monitor_now, "no monitors set")
        be.set_monitors({tag: None})
        be.monitor_now()
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        _state_error(hip, be.monitor_now, "no monitors set")
        assert be.monitor_count() == 0
    finally:
        prob.close()


# 9. the driver ----------------------------------------------------------------------------------------------------------------------------------
def test_run_simulation_with_a_monitors_block(hip, tmp_path):
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.run_with_diamond import run_simulation

    cfg = copy.deepcopy(load_cfg("geballe_with_diamond_source"))
    cfg["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in cfg["mats"].items()}
    cfg["timing"] = dict(cfg["timing"], num_steps=NSTEPS, t_final=NSTEPS * 7.5e-8)
    cfg["heating"]["source"]["pulse"] = {"t0": 7.5e-7, "fwhm": 6.0e-7}
    cfg["monitors"] = {"sample": {"material": "p_sample", "above": 301.0}, "coupler": {"material": ["p_coupler", "o_coupler"]}}
    out = tmp_path / "out"
    res = run_simulation(cfg, str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=str(out), watcher_points=get_watcher_points(cfg),
                         write_xdmf=False, suppress_print=True)
    m = res["monitors"]
    assert list(m) == ["sample", "coupler"] and all(len(v) == NSTEPS for f in m.values() for v in f.values())
    with open(out / "monitors.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert [float(r[0]) for r in rows[1:]] == [float(t) for t in res["times"]] and len(rows[0]) == 1 + sum(len(f) for f in m.values())
    for j, col in enumerate(rows[0][1:], start=1):
        region, field = col.split(".")
        assert [float(r[j]) for r in rows[1:]] == m[region][field].tolist(), col
    assert m["coupler"]["T_max"].max() > 310.0
    for name in ("pside", "oside"):        # the watchers sit on the couplers' faces: the region's peak is not below them
        assert np.all(m["coupler"]["T_max"] >= res["watchers"][name]), name
    assert "hot_volume" in m["sample"] and "hot_volume" not in m["coupler"] and "energy" in m["coupler"]
    assert m["sample"]["hot_fraction"].max() > 0.0 and np.all(m["sample"]["hot_fraction"] <= 1.0)
    assert np.all(np.diff(m["sample"]["energy"][:10]) > 0.0)              # the sample takes up heat while the pulse rises
