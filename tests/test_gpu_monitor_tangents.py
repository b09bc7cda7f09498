"""Derivatives of the region monitors in tangent runs on the GPU (hf_set_monitor_tangents, k_monitor_tan<NV>)
against the float64 restatement of tests/monitor_tangent_oracle.py: the kernels' own door row by row, repeatability, the records
of hf_run_tangent, the absence of side effects, central differences of GPU primal monitor runs, the error and state rules and the
driver.  Both small meshes, 20 steps at most."""
import copy
import csv
import functools
import re

import numpy as np
import pytest

import monitor_tangent_oracle as mto
from conftest import build_case, load_cfg
from helpers import material_tables, reference_bcs
from test_gpu_monitors import CASES, NSTEPS, _dt, _thresholds, _varying_state

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def small(which):
    return build_case(CASES[which], 8.0)


def _tangent_fields(n, nv, seed, zero_cols=()):
    s = np.random.default_rng(seed).standard_normal((n, nv)) * 25.0
    for j in zero_cols:
        s[:, j] = 0.0
    return s


def _velocities(mesh, cols, seed):
    """Smooth nodal z-velocities of order one (dz / dtheta of a thickness has that size) plus noise, one per column."""
    rng = np.random.default_rng(seed)
    z = np.asarray(mesh.coords)[:, 0]
    span = z.max() - z.min()
    return {int(j): (z - z.min()) / span * (0.5 + q) + 0.05 * rng.standard_normal(len(z)) for q, j in enumerate(cols)}


class _Grid:
    pass


@functools.lru_cache(maxsize=None)
def stripe_grid(stripes=5):
    """The 70 688-triangle grid of test_gpu_monitors (277 chunks on 272 workgroups), in ``stripes`` stripes of z: tags 1 .."""
    nz = nr = 188
    z, r = np.meshgrid(np.linspace(0.0, 4.0e-5, nz + 1), np.linspace(0.0, 2.0e-5, nr + 1), indexing="ij")
    coords = np.stack([z.ravel(), r.ravel()], axis=1)
    idx = np.arange((nz + 1) * (nr + 1)).reshape(nz + 1, nr + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    tris = np.stack([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)], axis=1).reshape(-1, 3).astype(np.int32)
    zc = coords[tris][:, :, 0].mean(axis=1)
    g = _Grid()
    g.coords, g.tris = coords, tris
    g.tags = (1 + np.minimum((zc / 4.0e-5 * stripes).astype(np.int32), stripes - 1)).astype(np.int32)
    assert len(tris) == 70688 and (len(tris) + 255) // 256 == 277
    return g


def _eval_and_check(be, mesh, u, th, s, shape, label):
    row = be.monitor_tangent_eval(s, shape)
    prim = be.monitor_now()
    ref, scale, ne = mto.per_tag_tangent(mesh.coords, mesh.tris, mesh.tags, u, th, s, shape, row.shape[0], primal=prim)
    worst = mto.check_row(row, ref, scale, ne, th, label)
    return row, worst


# 1. the kernels' own door against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nshape", [0, 1, 4])
@pytest.mark.parametrize("nv", [2, 16])
@pytest.mark.parametrize("which", sorted(CASES))
def test_eval_matches_the_restatement_row_by_row(hip, which, nv, nshape):
    _, _, mesh = small(which)
    th = _thresholds(mesh)
    u = _varying_state(mesh)
    zero = (1,) if nv == 2 else (3, 9)
    s = _tangent_fields(len(u), nv, 5 + nv, zero)
    cols = [0, 1, nv - 1, nv // 2][:nshape] if nv > 2 else [1, 0][:min(nshape, 2)]
    shape = _velocities(mesh, cols, 7)
    with hip.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_state(u)
        be.set_monitors(th)
        row, _ = _eval_and_check(be, mesh, u, th, s, shape, f"eval {which} nv={nv} shape={cols}")
        assert be.monitor_tangent_count() == (0, 0) and be.monitor_count() == 0          # nothing is recorded
    assert row.shape == (int(mesh.tags.max()) + 1, nv, 5)
    for j in zero:
        if j not in shape:
            assert np.all(row[:, j, :] == 0.0), j                                            # a column of zeros: exact zeros
    for j in range(nv):
        if j not in shape:
            assert np.all(row[:, j, 2] == 0.0)                                               # dI0 belongs to shape columns only
    for t, v in th.items():
        for j in range(nv):
            if j not in zero and j not in shape:
                assert row[t, j, 3] != 0.0 and (row[t, j, 4] != 0.0) == (v is not None), (t, j)


@pytest.mark.parametrize("nshape", [0, 4])
def test_eval_on_a_mesh_with_more_chunks_than_workgroups(hip, nshape):
    mesh = stripe_grid()
    th = {1: 420.0, 2: None, 4: 390.0, 5: 1.0e4}
    u = _varying_state(mesh, 31)
    s = _tangent_fields(len(u), 4, 41)
    shape = _velocities(mesh, [2, 0, 3, 1][:nshape], 43)
    with hip.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_state(u)
        be.set_monitors(th)
        row, _ = _eval_and_check(be, mesh, u, th, s, shape, f"eval grid 70688 nv=4 shape={sorted(shape)}")
        assert np.array_equal(row, be.monitor_tangent_eval(s, shape))
    assert np.all(row[3] == 0.0) and np.all(row[5, :, 4] == 0.0)                             # not monitored; nothing above 1e4 K


def test_eval_takes_the_columns_in_groups_when_the_accumulators_outgrow_the_lds(hip):
    """60 monitored tags and 16 columns: the accumulators of one launch (4 waves x 60 x 36 doubles) pass 64 KB, so the columns go
    in two launches of eight - the path no mesh of the project reaches."""
    mesh = stripe_grid(60)
    th = {t: (350.0 + 2.0 * t if t % 3 else None) for t in range(1, 61)}
    u = _varying_state(mesh, 33)
    s = _tangent_fields(len(u), 16, 47, (5,))
    shape = _velocities(mesh, [9, 2], 49)
    with hip.HeatflowHIP() as be:
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        be.set_state(u)
        be.set_monitors(th)
        row, _ = _eval_and_check(be, mesh, u, th, s, shape, "eval grid 70688, 60 tags, nv=16")
        s8 = np.ascontiguousarray(s[:, 8:])
        row8 = be.monitor_tangent_eval(s8, {1: shape[9]})
    assert np.all(row[:, 5, :] == 0.0)
    assert np.array_equal(row[:, 8:, :], row8)                                               # the second group: an nv = 8 call's bits


# 2. repeatability ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_two_contexts_and_the_other_columns(hip):
    _, _, mesh = small("no_diamond")
    th = _thresholds(mesh)
    u = _varying_state(mesh, 23)
    s = _tangent_fields(len(u), 4, 29)
    shape = _velocities(mesh, [1], 3)
    out = []
    for _ in range(2):
        with hip.HeatflowHIP() as be:
            be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
            be.set_state(u)
            be.set_monitors(th)
            first = be.monitor_tangent_eval(s, shape)
            assert np.array_equal(first, be.monitor_tangent_eval(s, shape))
            out.append(first)
            if len(out) == 2:
                # a column's result does not depend on what the other columns hold
                other = _tangent_fields(len(u), 4, 30)
                other[:, 1] = s[:, 1]
                other[:, 3] = s[:, 3]
                mixed = be.monitor_tangent_eval(other, shape)
                assert np.array_equal(mixed[:, [1, 3]], first[:, [1, 3]]) and not np.array_equal(mixed[:, 0], first[:, 0])
                # the same s_j in column 0 of an nv = 2 call and in column 3 of an nv = 4 call: within the bound (DESIGN.md 3.18:
                # the per-column operations and the order of the additions do not depend on nv, so the bits are expected equal)
                two = np.zeros((len(u), 2))
                two[:, 0] = s[:, 3]
                narrow = be.monitor_tangent_eval(two)
                ref, scale, ne = mto.per_tag_tangent(mesh.coords, mesh.tris, mesh.tags, u, th, two, None, first.shape[0],
                                                     primal=be.monitor_now())
                bound = mto.sum_bound(ne, scale)[:, 0, :]
                diff = np.abs(narrow[:, 0, 2:] - first[:, 3, 2:])
                print(f"column 0 of nv = 2 against column 3 of nv = 4: largest difference {diff.max():.3e} "
                      f"(bitwise equal: {np.array_equal(narrow[:, 0], first[:, 3])})")
                assert np.all(diff <= 2.0 * bound) and np.array_equal(narrow[:, 0, :2], first[:, 3, :2])
    assert np.array_equal(out[0], out[1])


# 3. the records of hf_run_tangent ----------------------------------------------------------------------------------------------------------------
def _problem(case, precond, scheme, rtol=None, **kw):
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = case
    tk, trc = material_tables(stack, mesh)
    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    prob = HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, _dt(cfg), bcs, ic, precond=precond, scheme=scheme,
                       **({"rtol": rtol} if rtol else {}), **kw)
    prob.backend.set_monitors(_thresholds(mesh))
    return prob


def _columns(case, kind):
    """(HeatProblem keywords, run_tangent keywords, {column: velocity}) of one kind of tangent columns."""
    from heatflow_amd.geometry import thickness_velocity

    cfg, _, mesh = case
    tag = mesh.material_tags["p_sample"]
    if kind == "k+rho_c":          # a conductivity column and a capacity column on the sample
        return {}, {"conductivity": [[tag], []], "capacity": [[], [tag]]}, {}
    if kind == "thickness":        # a shape column
        v = thickness_velocity(cfg, "p_sample", mesh.coords[:, 0])
        return {}, {"conductivity": [[]], "shape": {0: v}}, {0: v}
    return {"k_aniso": {tag: (2.0, 1.0)}}, {"conductivity": [[(tag, "r")], [(tag, "z")]]}, {}      # directional columns


FIRST = 14          # the steps start at 1.1 us, where the heating curve begins to rise: the tangents are not noise
RUN_CASES = [(kind, which, precond, scheme) for kind in ("k+rho_c", "thickness", "directional")
             for which, precond, scheme in (("with_diamond", 1, "backward_euler"), ("no_diamond", 0, "bdf2"),
                                            ("with_diamond", 0, "bdf2"), ("no_diamond", 1, "backward_euler"))]


@pytest.mark.parametrize("kind, which, precond, scheme", RUN_CASES)
def test_every_step_of_hf_run_tangent_leaves_the_derivatives_of_its_state(hip, kind, which, precond, scheme):
    case = small(which)
    _, _, mesh = case
    th = _thresholds(mesh)
    pkw, rkw, shape = _columns(case, kind)
    prob = _problem(case, precond, scheme, **pkw)
    be = prob.backend
    worst = np.zeros(3)
    try:
        be.set_monitor_tangents(True)
        for k in range(5):                                                  # one step per call: the tangents continue
            prob.run_tangent(1, None, time_varying=prob.bcs[3:], first_step=FIRST + k, **rkw)
            nv = be.tangent_nv
            assert be.monitor_tangent_count() == (k + 1, nv) and be.monitor_count() == k + 1
            drec, index = be.get_monitor_tangents(k, 1)
            assert index.tolist() == [k] and drec.shape == (1, int(mesh.tags.max()) + 1, nv, 5)
            u = be.get_state()
            s = np.stack([be.get_tangent(j) for j in range(nv)], axis=1)
            prim = be.get_monitors(k, 1)[0]
            ref, scale, ne = mto.per_tag_tangent(mesh.coords, mesh.tris, mesh.tags, u, th, s, shape, drec.shape[1], primal=prim)
            worst = np.maximum(worst, mto.check_row(drec[0], ref, scale, ne, th, f"hf_run_tangent {kind} {which} precond={precond} {scheme} step {k}"))
        assert np.abs(s[:, 0]).max() > 0.0 and drec[0][mesh.material_tags["p_sample"], 0, 3] != 0.0      # (the heated line shields the p-side insulation)
        if nv > len(rkw["conductivity"]):
            assert np.all(drec[0][:, len(rkw["conductivity"]):, :] == 0.0)   # padded columns: zero tangents, zero derivatives
        prob.run_tangent(NSTEPS, None, time_varying=prob.bcs[3:], first_step=FIRST + 5, **rkw)
        assert be.monitor_tangent_count() == (5 + NSTEPS, nv) and be.monitor_count() == 5 + NSTEPS
        drec, index = be.get_monitor_tangents()
        assert index.tolist() == list(range(5 + NSTEPS))
        s = np.stack([be.get_tangent(j) for j in range(nv)], axis=1)
        assert np.array_equal(drec[-1], be.monitor_tangent_eval(s, shape))    # bit for bit the kernels' own door on the final fields
        assert np.array_equal(be.get_monitor_tangents(7, 3)[0], drec[7:10])
    finally:
        prob.close()
    print(f"hf_run_tangent {kind} {which} precond={precond} {scheme}: worst error / bound over 5 steps {worst}")


# 4. no side effects ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, precond", [("k+rho_c", 1), ("thickness", 0)])
def test_the_derivative_records_change_nothing_else(hip, kind, precond):
    case = small("with_diamond")
    _, _, mesh = case
    pkw, rkw, _ = _columns(case, kind)
    runs = []
    for on in (False, True):
        prob = _problem(case, precond, "backward_euler", **pkw)
        nodes = np.arange(prob.n, dtype=np.int32)
        try:
            if on:
                prob.backend.set_monitor_tangents(True)
            _, s, ts, it, tit = prob.run_tangent(NSTEPS, nodes, time_varying=prob.bcs[3:], **rkw)
            runs.append((s, ts, it, tit, prob.state(), prob.tangent(0), prob.backend.get_monitors()))
            assert prob.backend.monitor_tangent_count()[0] == (NSTEPS if on else 0)
        finally:
            prob.close()
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert np.abs(runs[0][1]).max() > 0.0


# 5. central differences of GPU primal monitor runs ------------------------------------------------------------------------------------------------
def _fd_cfg(which):
    cfg = copy.deepcopy(small(which)[0])
    cfg["timing"] = dict(cfg["timing"], num_steps=mto.FD_NSTEPS, t_final=mto.FD_T_FINAL)
    cfg["monitors"] = copy.deepcopy(mto.FD_MONITORS)
    return cfg


def _gpu_session(mesh):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, rtol=1e-12, precond=1)


def test_derivatives_match_central_differences_of_gpu_monitor_runs(hip):
    """Multigrid at rtol = 1e-12; the run, the regions and the relative steps are the ones tests/test_monitor_tangents_cpu.py
    recorded in float64 (monitor_tangent_oracle.FD_*)."""
    from types import SimpleNamespace

    from heatflow_amd.fit import get_param, set_params
    from heatflow_amd.geometry import build_stack, thickness_velocity

    _, _, mesh = small("with_diamond")
    cfg = _fd_cfg("with_diamond")
    names = list(mto.FD_REL_STEP)

    def run(c, m, **kw):
        s = _gpu_session(m)
        try:
            res = s.run(c, build_stack(c), None, **kw)
            return res, s.problem.backend.get_monitors()
        finally:
            s.close()

    res, base = run(cfg, mesh, tangents=names, monitor_tangents=True)
    for name in names:
        t0, rel = get_param(cfg, name), mto.FD_REL_STEP[name]
        sides = []
        for sg in (1.0, -1.0):
            value = t0 * (1.0 + sg * rel)
            c, m = set_params(cfg, (name,), (value,)), mesh
            if name.endswith(".thickness"):
                coords = np.array(mesh.coords, dtype=np.float64)
                coords[:, 0] += thickness_velocity(cfg, name.rsplit(".", 1)[0], mesh.coords[:, 0]) * (value - t0)
                m = SimpleNamespace(coords=coords, tris=mesh.tris, tags=mesh.tags, material_tags=mesh.material_tags)
            r, rec = run(c, m)
            assert np.array_equal(rec[:, :, 1], base[:, :, 1]), name           # the peak's node is the same in the three runs
            sides.append(r["monitors"])
        for region in ("sample", "coupler"):
            for field in ("T_mean", "energy", "T_max"):
                d = res["monitor_tangents"][name][region][field]
                fd = (sides[0][region][field] - sides[1][region][field]) / (2.0 * rel * t0)
                scale, err = float(np.max(np.abs(d))), float(np.max(np.abs(d - fd)))
                print(f"{name} {region}.{field}: max |d| theta = {scale * t0:.3e}; |d - FD| / max|d| = {err / scale:.2e} at relative step {rel:g}")
                assert scale > 0.0 and err <= mto.FD_TOL * scale, (name, region, field)


# 6. errors and lifetime -----------------------------------------------------------------------------------------------------------------------------
def _state_error(hip, fn, pattern):
    with pytest.raises(hip.HipError, match=pattern) as ei:
        fn()
    assert ei.value.code == hip.HF_ERR_STATE


def test_error_returns_and_lifetime(hip):
    import ctypes as C

    case = small("with_diamond")
    _, _, mesh = case
    tag, other = mesh.material_tags["p_sample"], mesh.material_tags["p_ins"]
    tab_len = int(mesh.tags.max()) + 1
    n = len(mesh.coords)
    with hip.HeatflowHIP() as be:
        be.tab_len, be.n = tab_len, n
        _state_error(hip, lambda: be.set_monitor_tangents(True), "hf_set_monitor_tangents before hf_set_mesh")
        _state_error(hip, be.monitor_tangent_count, "hf_monitor_tangent_count before hf_set_mesh")
        _state_error(hip, lambda: be.monitor_tangent_eval(np.zeros((n, 2))), "hf_monitor_tangent_eval before hf_set_mesh")
        assert be._lib.hf_get_monitor_tangents(be._ctx, 0, 0, None, None) == hip.HF_ERR_STATE     # (the wrapper asks for the count first)
        assert re.search("hf_get_monitor_tangents before hf_set_mesh", be._lib.hf_last_error(be._ctx).decode())
    prob = _problem(case, 0, "backward_euler")
    be = prob.backend
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    try:
        be.set_monitors({})
        _state_error(hip, lambda: be.set_monitor_tangents(True), r"hf_set_monitor_tangents: no monitors set \(hf_set_monitors first\)")
        be.set_monitor_tangents(False)                                      # switching off needs nothing
        _state_error(hip, lambda: be.get_monitor_tangents(0, 0), r"hf_get_monitor_tangents: no monitors set")
        _state_error(hip, lambda: be.monitor_tangent_eval(np.zeros((n, 2))), r"hf_monitor_tangent_eval: no monitors set")
        assert be.monitor_tangent_count() == (0, 0)
        be.set_monitors({tag: 350.0})
        # argument rules of the kernels' own door
        s2 = np.zeros((n, 2))
        v = np.zeros(n)
        for nv in (1, 3, 5, 32, 0):
            with pytest.raises(ValueError, match=rf"hf_monitor_tangent_eval: nv = {nv} \(2, 4, 8 or 16 columns\)"):
                be.monitor_tangent_eval(np.zeros((n, nv)))
        with pytest.raises(ValueError, match=r"hf_monitor_tangent_eval: shape column 2 outside \[0,2\)"):
            be.monitor_tangent_eval(s2, {2: v})
        with pytest.raises(ValueError, match=r"hf_monitor_tangent_eval: shape column -1 outside \[0,2\)"):
            be.monitor_tangent_eval(s2, {-1: v})
        s8 = np.zeros((n, 8))
        with pytest.raises(ValueError, match=r"hf_monitor_tangent_eval: 5 shape columns \(0\.\.4\)"):
            be.monitor_tangent_eval(s8, {j: v for j in range(5)})
        out = np.zeros((tab_len, 2, 5))
        cols = np.array([1, 1], dtype=np.int32)
        vz = np.zeros((n, 2))
        lib, ctx = be._lib, be._ctx
        assert lib.hf_monitor_tangent_eval(ctx, 2, s2.ctypes.data_as(pd), 2, cols.ctypes.data_as(pi), vz.ctypes.data_as(pd),
                                           out.ctypes.data_as(pd)) == hip.HF_ERR_ARG
        assert re.search(r"hf_monitor_tangent_eval: shape column 1 is listed twice", lib.hf_last_error(ctx).decode())
        for args in ((2, None, 0, None, None, out.ctypes.data_as(pd)), (2, s2.ctypes.data_as(pd), 0, None, None, None),
                     (2, s2.ctypes.data_as(pd), 1, None, vz.ctypes.data_as(pd), out.ctypes.data_as(pd)),
                     (2, s2.ctypes.data_as(pd), 1, cols.ctypes.data_as(pi), None, out.ctypes.data_as(pd))):
            assert lib.hf_monitor_tangent_eval(ctx, *args) == hip.HF_ERR_ARG
            assert re.search(r"hf_monitor_tangent_eval: null pointer", lib.hf_last_error(ctx).decode())
        assert lib.hf_monitor_tangent_count(ctx, None, None) == hip.HF_ERR_ARG
        assert re.search(r"hf_monitor_tangent_count: null pointer", lib.hf_last_error(ctx).decode())
        # records: three steps of a tangent run with the switch on, none with it off
        kw = {"conductivity": [[tag]], "time_varying": prob.bcs[3:]}
        prob.run_tangent(2, None, **kw)
        assert be.monitor_tangent_count() == (0, 0) and be.monitor_count() == 2
        be.set_monitor_tangents(True)
        prob.run_tangent(3, None, first_step=2, **kw)
        assert be.monitor_tangent_count() == (3, 2) and be.monitor_count() == 5
        drec, index = be.get_monitor_tangents()
        assert index.tolist() == [2, 3, 4]                                 # the primal records of hf_run / hf_step come in between
        g = prob.bc_values(6 * prob.dt)
        be.step(g)
        prob.run_tangent(1, None, first_step=6, **kw)
        assert be.get_monitor_tangents()[1].tolist() == [2, 3, 4, 6] and be.monitor_count() == 7
        for first, count, pat in ((0, 5, r"hf_get_monitor_tangents: records \[0, 5\) outside the 4 derivative records kept"),
                                  (-1, 1, r"records \[-1, 0\) outside"), (4, 1, r"records \[4, 5\) outside"), (1, -1, r"records \[1, 0\) outside")):
            with pytest.raises(ValueError, match=pat):
                be.get_monitor_tangents(first, count)
        assert be.get_monitor_tangents(4, 0)[0].shape == (0, tab_len, 2, 5)
        assert lib.hf_get_monitor_tangents(ctx, 0, 1, None, None) == hip.HF_ERR_ARG
        assert re.search(r"hf_get_monitor_tangents: null pointer for records \[0, 1\)", lib.hf_last_error(ctx).decode())
        one = np.zeros((1, tab_len, 2, 5))
        assert lib.hf_get_monitor_tangents(ctx, 3, 1, one.ctypes.data_as(pd), None) == hip.HF_OK      # record_index may be NULL
        assert np.array_equal(one[0], be.get_monitor_tangents()[0][3])
        # a step that fails leaves no record of either kind
        with pytest.raises(hip.NotConverged):
            be.run_tangent(np.stack([g + 50.0]), None, prob.rtol, 0.0, 1, None)
        assert be.monitor_tangent_count() == (4, 2) and be.monitor_count() == 7
        # hf_monitor_clear drops both kinds and keeps the switch
        be.clear_monitor_records()
        assert be.monitor_tangent_count()[0] == 0 and be.monitor_count() == 0
        prob.run_tangent(2, None, first_step=7, **kw)
        assert be.monitor_tangent_count() == (2, 2) and be.get_monitor_tangents()[1].tolist() == [0, 1]
        # a set-up with another nv drops the derivative records (their rows have nv columns), not the primal ones; one with the same nv keeps them
        prob.run_tangent(1, None, conductivity=[[other]], time_varying=prob.bcs[3:])
        assert be.monitor_tangent_count() == (3, 2) and be.monitor_count() == 3
        prob.run_tangent(1, None, conductivity=[[tag], [other], []], time_varying=prob.bcs[3:])
        assert be.monitor_tangent_count() == (1, 4) and be.monitor_count() == 4 and be.get_monitor_tangents()[1].tolist() == [3]
        # hf_set_monitors switches off and drops the records; so does hf_set_mesh
        be.set_monitors({tag: 350.0, other: None})
        assert be.monitor_tangent_count() == (0, 0)
        prob.run_tangent(1, None, conductivity=[[tag], [other], []], time_varying=prob.bcs[3:])
        assert be.monitor_tangent_count() == (0, 0) and be.monitor_count() == 1
        be.set_monitor_tangents(True)
        prob.run_tangent(1, None, conductivity=[[tag], [other], []], time_varying=prob.bcs[3:])
        assert be.monitor_tangent_count() == (1, 4)
        # an open batch refuses
        be.batch_begin(2)
        for fn, name in ((lambda: be.set_monitor_tangents(True), "hf_set_monitor_tangents"), (be.monitor_tangent_count, "hf_monitor_tangent_count"),
                         (lambda: be.monitor_tangent_eval(s2), "hf_monitor_tangent_eval")):
            _state_error(hip, fn, rf"{name}: a batch is open")
        assert lib.hf_get_monitor_tangents(ctx, 0, 1, one.ctypes.data_as(pd), None) == hip.HF_ERR_STATE
        assert re.search("hf_get_monitor_tangents: a batch is open", lib.hf_last_error(ctx).decode())
        be.batch_end()
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        assert be.monitor_tangent_count() == (0, 0)
        _state_error(hip, lambda: be.set_monitor_tangents(True), "no monitors set")
    finally:
        prob.close()


# 7. the driver ------------------------------------------------------------------------------------------------------------------------------------
def test_run_simulation_with_monitor_sigma(hip, tmp_path):
    from heatflow_amd.fit import get_param
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.run_with_diamond import run_simulation

    cfg = copy.deepcopy(load_cfg("geballe_with_diamond"))
    cfg["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in cfg["mats"].items()}
    cfg["timing"] = dict(cfg["timing"], num_steps=NSTEPS, t_final=7.5e-6)
    cfg["monitors"] = {"sample": {"material": "p_sample", "above": 301.0}, "coupler": {"material": ["p_coupler", "o_coupler"]}}
    sigma = {"p_sample.rho_c": 0.15, "p_ins.rho_c": 0.15, "p_sample.thickness": 0.05, "fwhm": 0.1}
    out = tmp_path / "out"
    res = run_simulation(cfg, str(tmp_path / "mesh"), rebuild_mesh=True, output_folder=str(out), watcher_points=get_watcher_points(cfg),
                         write_xdmf=False, suppress_print=True, monitor_sigma=sigma)
    assert list(res["monitor_tangents"]) == list(sigma) and list(res["monitor_uncertainty"]) == ["sample", "coupler"]
    m, band, mt = res["monitors"], res["monitor_uncertainty"], res["monitor_tangents"]
    assert all(len(v) == NSTEPS for f in band.values() for v in f.values())
    for region in band:
        want = np.sqrt(sum((mt[q][region]["T_mean"] * sg * get_param(cfg, q)) ** 2 for q, sg in sigma.items()))
        print(f"{region}: T_mean {m[region]['T_mean'][-1]:.3f} K +- {band[region]['T_mean'][-1]:.3f} K at the last step; per parameter "
              + ", ".join(f"{q} {mt[q][region]['T_mean'][-1] * sg * get_param(cfg, q):+.3e}" for q, sg in sigma.items()))
        assert np.allclose(band[region]["T_mean"], want, rtol=1e-14, atol=0.0) and band[region]["T_mean"].max() > 0.0
    assert "hot_fraction" in band["sample"] and "hot_fraction" not in band["coupler"] and "energy" in band["coupler"]
    with open(out / "monitor_uncertainty.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert [float(r[0]) for r in rows[1:]] == [float(t) for t in res["times"]]
    head = rows[0][1:]
    assert head[1::2] == [c + ".sigma" for c in head[0::2]] and "sample.hot_fraction" in head and "coupler.T_mean.sigma" in head
    for j, col in enumerate(head, start=1):
        region, field = col.split(".")[:2]
        assert [float(r[j]) for r in rows[1:]] == np.asarray((band if col.endswith(".sigma") else m)[region][field]).tolist(), col
    with open(out / "monitors.csv", newline="") as f:
        assert next(csv.reader(f)) == ["time"] + [f"{r}.{f}" for r in m for f in mon_fields(m[r])]


def mon_fields(fields):
    from heatflow_amd.monitors import FIELDS

    return [f for f in FIELDS if f in fields]
