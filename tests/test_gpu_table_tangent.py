"""Tangent runs under kappa(T) / rho_c(T) tables on the GPU (hf_table_derivatives, hf_tangent_set_tables, k_tangent_load_T; DESIGN.md
3.20): the load row by row against the restatement (table_tangent_oracle.py) for every width, the exact recursion, central
differences of GPU primal runs, the bitwise promises, every error return, and the driver and the fit end to end."""
import copy
import json

import numpy as np
import pytest

from conftest import HEATING_CSV
from helpers import make_problem, material_tables
from kappa_T_oracle import element_temperature, problem_inputs
from rhoc_T_oracle import einstein_tables
from table_tangent_oracle import BDF2, BE, FD_REL_STEP, _tag_matrix, table_term, tangent_fields, unit_rows

pytestmark = pytest.mark.gpu

NSTEPS = 20


def _heat(cfg):
    from heatflow_amd.heating import HeatingCurve

    return HeatingCurve(HEATING_CSV, float(cfg["heating"]["ic_temp"]), float(cfg["heating"]["fwhm"]))


def _wide_field(mesh):
    """150 .. 1050 K: a swing along r with the period of the sample chamber (every thin layer sees all of it, and it survives three
    steps), modulated along z, under nodal noise."""
    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    rng = np.random.default_rng(11)
    smooth = np.cos(np.pi * r / 20e-6) * (1.0 - 0.1 * np.sin(7.0 * (z - z.min()) / (z.max() - z.min())))
    return 600.0 + 400.0 * smooth + 10.0 * (2.0 * rng.random(len(z)) - 1.0)


# 1. the load -----------------------------------------------------------------------------------------------------------------------------
def _load_tables(mesh, tk, trc, knots):
    """Two tabled tags with different grids: the p-side insulator on ``knots`` knots over 310..400 K (conductivity and capacity), the
    o-side insulator on 37 knots over 340..520 K (conductivity only).  Values with slopes of both signs.  (Without diamonds the
    insulators' outer faces are held at 300 K, and three steps pull the thin p-side layer down to 280..470 K.)"""
    t = mesh.material_tags
    Tp = np.linspace(310.0, 400.0, knots)
    To = 340.0 + 5.0 * np.arange(37)
    kt = {t["p_ins"]: (310.0, 90.0 / (knots - 1), tk[t["p_ins"]] * (1.0 + 0.4 * np.sin(Tp / 40.0) + (Tp - 310.0) / 400.0)),
          t["o_ins"]: (340.0, 5.0, tk[t["o_ins"]] * 340.0 / To)}
    ct = {t["p_ins"]: (310.0, 90.0 / (knots - 1), trc[t["p_ins"]] * (1.0 + 0.3 * np.cos(Tp / 55.0)))}
    return kt, ct


@pytest.mark.parametrize("ncol,knots,scheme", [(1, 2, "backward_euler"), (3, 256, "bdf2"), (5, 2, "bdf2"), (9, 256, "backward_euler")])
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_load_after_three_steps_row_by_row(hip, request, case, ncol, knots, scheme):
    """hf_tangent_load after three steps against the restatement at the GPU's own u, u^n, u^{n-1} and columns: every row within 1e-13
    of the sum of its terms' magnitudes.  Column 0 carries D tables of both kinds on both tags; column 1 (ncol >= 3) is p_sample's
    conductivity, which meets the tables through the coupling term alone; column 2 a D on the o side only; the rest repeat
    these with other values.  Padded columns are exact zeros, rows that touch no tabled element keep the bits they have without
    the tables' term."""
    cfg, stack, mesh = request.getfixturevalue(case)
    t = mesh.material_tags
    tk, trc = material_tables(stack, mesh)
    kt, ct = _load_tables(mesh, tk, trc, knots)
    p_ins, o_ins, sample = t["p_ins"], t["o_ins"], t["p_sample"]
    rng = np.random.default_rng(5)
    Dk, Dc, cond = {}, {}, [[] for _ in range(ncol)]
    for j in range(ncol):
        if j % 3 == 0:
            Dk[(j, p_ins)] = kt[p_ins][2] * rng.normal(size=knots)
            Dk[(j, o_ins)] = kt[o_ins][2] * (1.0 + j)
            Dc[(j, p_ins)] = ct[p_ins][2] * rng.normal(size=knots)
        elif j % 3 == 1:
            cond[j] = [{1: sample, 4: t["p_coupler"], 7: t["o_coupler"]}[j]]
        else:
            Dk[(j, o_ins)] = -kt[o_ins][2] * np.log(340.0 / (340.0 + 5.0 * np.arange(37)) + 1.5)
    tables = {}
    for q, D in (("kappa", Dk), ("rhoc", Dc)):
        for (j, tag), v in D.items():
            tables.setdefault(j, {}).setdefault(q, {})[tag] = v
    nv = next(v for v in (2, 4, 8, 16) if v >= ncol)
    prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme, kappa_tables=kt, rhoc_tables=ct)
    try:
        prob.set_state(_wide_field(mesh))
        states, cols = [prob.state()], []
        for k in range(3):
            prob.run_tangent(1, None, conductivity=cond, tables=tables, time_varying=[prob.bcs[3]], first_step=k)
            states.append(prob.state())
            cols.append(np.stack([prob.tangent(j) for j in range(ncol)], axis=1))
        assert prob.backend.tangent_nv == nv
        got = [prob.tangent_load(j) for j in range(nv)]
    finally:
        prob.close()
    # the same state on a problem without tables: the bits of the conductivity columns' -K_j u
    plain = make_problem(cfg, stack, mesh, precond=1, scheme=scheme)
    try:
        plain.backend.tangent_setup(ncol, {tag: j for j, tags in enumerate(cond) for tag in tags})
        plain.set_state(states[3])
        base = [plain.tangent_load(j) for j in range(ncol)]
    finally:
        plain.close()
    u, un, um1 = states[3], states[2], states[1]
    bdf2 = scheme == "bdf2"
    dtp = 2.0 * prob.dt / 3.0 if bdf2 else prob.dt
    w = ((u - (4.0 / 3.0) * un) + (1.0 / 3.0) * um1) / dtp if bdf2 else (u - un) / dtp
    ustar = 2.0 * un - um1 if bdf2 else un
    sstar = 2.0 * cols[2] - cols[1] if bdf2 else cols[2]         # the columns as they stand after the run
    rows = unit_rows(mesh.coords, mesh.tris)
    F, mag = table_term(mesh.coords, mesh.tris, mesh.tags, kt, ct, Dk, Dc, ncol, u, w, ustar, sstar, rows=rows)
    # both clamped ranges and the interior segments hold tabled elements
    Te = element_temperature(ustar, np.asarray(mesh.tris))
    tags = np.asarray(mesh.tags)
    for tag, lo, hi in ((p_ins, 310.0, 400.0), (o_ins, 340.0, 520.0)):
        T = Te[tags == tag]
        assert (T <= lo).sum() > 10 and (T >= hi).sum() > 10 and ((T > lo) & (T < hi)).sum() > 10, (tag, T.min(), T.max())
    touched = np.zeros(len(mesh.coords), dtype=bool)
    touched[np.asarray(mesh.tris)[np.isin(tags, [p_ins, o_ins])].ravel()] = True
    assert touched.any() and (~touched).sum() > 100
    worst = 0.0
    for j in range(ncol):
        ref, T = F[:, j].copy(), mag[:, j].copy()
        if cond[j]:
            K = _tag_matrix(len(mesh.coords), mesh.tris, mesh.tags, rows[1], cond[j])
            ref -= K @ u
            T += abs(K) @ np.abs(u)
        assert np.array_equal(got[j][~touched], base[j][~touched]), j       # no tabled element: the bits of before
        assert np.any(F[touched, j] != 0.0), j                             # ... and the term is live where there is one
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(T > 0, np.abs(got[j] - ref) / T, np.where(got[j] == 0, 0.0, np.inf))
        worst = max(worst, float(ratio.max()))
        assert np.max(np.abs(F[:, j]) / np.where(T > 0, T, np.inf)) > 1e-3, j   # the term is not small against its terms everywhere
    for j in range(ncol, nv):
        assert not got[j].any(), j                                          # padded columns: exact zeros
    print(f"{case} {scheme} ncol={ncol} nv={nv} knots={knots}: max |F - ref| / sum |terms| = {worst:.2e}")
    assert worst <= 1e-13


# 2. the exact recursion ------------------------------------------------------------------------------------------------------------------
def _recursion_tables(mesh, tk, trc):
    """The tables of tests/test_table_tangent_cpu.py: 1/T on both insulators (11 knots to 400 K on the p side, 51 to 800 K on the o
    side), Einstein capacities on both."""
    t = mesh.material_tags
    ins = [t["p_ins"], t["o_ins"]]
    Tp, To = 300.0 + 10.0 * np.arange(11), 300.0 + 10.0 * np.arange(51)
    kt = {ins[0]: (300.0, 10.0, tk[ins[0]] * 300.0 / Tp), ins[1]: (300.0, 10.0, tk[ins[1]] * 300.0 / To)}
    return ins, kt, einstein_tables(trc, ins), Tp


def _recursion_columns(mesh, ins, kt, ct, Tp):
    """Columns: the k table scale of both insulators, a p_ins.k_power.exponent-style D, the cv table scale, p_sample's k, fwhm."""
    Dk = {**{(0, tg): kt[tg][2] for tg in ins}, (1, ins[0]): kt[ins[0]][2] * np.log(300.0 / Tp)}
    Dc = {(2, tg): ct[tg][2] for tg in ins}
    tables = {0: {"kappa": {tg: kt[tg][2] for tg in ins}}, 1: {"kappa": {ins[0]: Dk[(1, ins[0])]}}, 2: {"rhoc": {tg: ct[tg][2] for tg in ins}}}
    cond = [[], [], [], [mesh.material_tags["p_sample"]], []]
    return Dk, Dc, tables, cond


NAMES = ["ins k table scale", "p_ins exponent", "ins cv table scale", "p_sample k", "fwhm"]


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_tangents_match_the_exact_recursion(hip, request, case, scheme):
    cfg, stack, mesh = request.getfixturevalue(case)
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, NSTEPS)
    ins, kt, ct, Tp = _recursion_tables(mesh, tk, trc)
    Dk, Dc, tables, cond = _recursion_columns(mesh, ins, kt, ct, Tp)
    nodes = np.sort(np.random.default_rng(0).choice(len(mesh.coords), 12, replace=False)).astype(np.int32)
    ref = None
    for precond in (0, 1):
        prob = make_problem(cfg, stack, mesh, precond=precond, scheme=scheme, kappa_tables=kt, rhoc_tables=ct)
        seen = {}
        inner = prob.backend.run_tangent

        def record(g_all, h_all=None, *a, **kw):
            seen["g"], seen["h"] = np.array(g_all), np.array(h_all)
            return inner(g_all, h_all, *a, **kw)

        prob.backend.run_tangent = record
        try:
            _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=cond, boundary={4: {3: _heat(cfg).gaussian_dfwhm}},
                                              tables=tables, time_varying=[prob.bcs[3]])
            fields = [prob.tangent(j) for j in range(5)]
            final = prob.state()
        finally:
            prob.close()
        if ref is None:       # the restatement once per case and scheme, with the boundary tables the GPU run was given
            assert seen["g"].shape == g.shape and np.abs(seen["g"] - g).max() <= 1e-9
            ref = tangent_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, seen["g"], kt, ct, BDF2 if scheme == "bdf2" else BE,
                                 ncol=5, conductivity={3: cond[3]}, Dk=Dk, Dc=Dc, h_all=seen["h"][:, :, :5])
            tags = np.asarray(mesh.tags)
            hot = np.unique(np.asarray(mesh.tris)[np.isin(tags, ins)])
            assert ref[0][-1][hot].max() - 300.0 > 100.0          # the tabled materials heat: the coupling term is live
        assert np.abs(final - ref[0][-1]).max() <= 1e-4
        for j, nm in enumerate(NAMES):
            s_ref = ref[1][:, j]
            scale = np.max(np.abs(s_ref))
            assert scale > 0
            err_s = np.max(np.abs(ts[:, j] - s_ref[:, nodes])) / scale
            err_f = np.max(np.abs(fields[j] - s_ref[-1])) / scale
            print(f"{case} {scheme} precond={precond} {nm}: samples off by {err_s:.2e}, final field by {err_f:.2e} of max|s|")
            assert err_s <= 1e-6 and err_f <= 1e-6, (case, scheme, precond, nm)


# 3. central differences of GPU primal runs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k_table.scale", "cv_table.scale"])
def test_tangents_match_central_differences_of_gpu_runs(hip, case_with_diamond_small, name):
    """Multigrid at rtol = 1e-12; the relative step is the one tests/test_table_tangent_cpu.py found in float64."""
    cfg, stack, mesh = case_with_diamond_small
    tk, trc = material_tables(stack, mesh)
    ins, kt, ct, Tp = _recursion_tables(mesh, tk, trc)
    nodes = np.arange(0, len(mesh.coords), max(1, len(mesh.coords) // 50), dtype=np.int32)
    rel = FD_REL_STEP[name]
    cap = name == "cv_table.scale"

    def scaled(tabs, f):
        return {tg: (a, b, f * v) for tg, (a, b, v) in tabs.items()}

    prob = make_problem(cfg, stack, mesh, precond=1, rtol=1e-12, kappa_tables=kt, rhoc_tables=ct)
    try:
        own = ct if cap else kt
        _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, tables={0: {"rhoc" if cap else "kappa": {tg: own[tg][2] for tg in ins}}},
                                          time_varying=[prob.bcs[3]])
        s = ts[:, 0]
    finally:
        prob.close()
    runs = []
    for sg in (1, -1):
        f = 1 + sg * rel
        prob = make_problem(cfg, stack, mesh, precond=1, rtol=1e-12, kappa_tables=kt if cap else scaled(kt, f),
                            rhoc_tables=scaled(ct, f) if cap else ct)
        try:
            runs.append(prob.run(NSTEPS, nodes, time_varying=[prob.bcs[3]])[1])
        finally:
            prob.close()
    fd = (runs[0] - runs[1]) / (2 * rel)
    scale = float(np.max(np.abs(s)))
    err = float(np.max(np.abs(s - fd)))
    print(f"{name}: max |s| = {scale:.3e} K; |s - FD| / max|s| = {err / scale:.2e} at relative step {rel:g}")
    assert scale > 0 and err <= 1e-4 * scale


# 4. bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_primal_under_tables_is_bitwise_that_of_hf_run(hip, case_with_diamond_small, scheme):
    cfg, stack, mesh = case_with_diamond_small
    tk, trc = material_tables(stack, mesh)
    ins, kt, ct, Tp = _recursion_tables(mesh, tk, trc)
    _, _, tables, cond = _recursion_columns(mesh, ins, kt, ct, Tp)
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    out = []
    for tangent in (False, True):
        prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme, kappa_tables=kt, rhoc_tables=ct)
        try:
            if tangent:
                kw = dict(conductivity=cond[:4], tables=tables, time_varying=[prob.bcs[3]])
                _, s1, _, it1, _ = prob.run_tangent(12, nodes, **kw)
                _, s2, _, it2, _ = prob.run_tangent(6, nodes, first_step=12, **kw)
            else:
                _, s1, it1 = prob.run(12, nodes, time_varying=[prob.bcs[3]])
                _, s2, it2 = prob.run(6, nodes, time_varying=[prob.bcs[3]], first_step=12)
            out.append((s1, it1, s2, it2, prob.state()))
        finally:
            prob.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_two_calls_and_two_contexts_give_the_same_bits(hip, case_with_diamond_small, scheme):
    cfg, stack, mesh = case_with_diamond_small
    tk, trc = material_tables(stack, mesh)
    ins, kt, ct, Tp = _recursion_tables(mesh, tk, trc)
    _, _, tables, cond = _recursion_columns(mesh, ins, kt, ct, Tp)
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    out = []
    for _ in range(2):
        prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme, kappa_tables=kt, rhoc_tables=ct)
        try:
            _, s, ts, it, tit = prob.run_tangent(15, nodes, conductivity=cond[:4], tables=tables, time_varying=[prob.bcs[3]])
            first = [prob.tangent_load(j) for j in range(4)]
            second = [prob.tangent_load(j) for j in range(4)]
            for a, b in zip(first, second):
                assert np.array_equal(a, b) and a.any()
            out.append([s, ts, it, tit] + first + [prob.tangent(j) for j in range(4)])
        finally:
            prob.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
def test_constant_tables_reproduce_the_linear_tangents(hip, case_with_diamond_small, scheme):
    """Tables of slope 0 and no D: the tangents of the linear run with the opt-in off, to 1e-9 of max|s| (the iterates differ only
    through the start vector; both runs solve to rtol = 1e-13)."""
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    tk, trc = material_tables(stack, mesh)
    kt = {t["p_ins"]: (300.0, 500.0, np.full(2, tk[t["p_ins"]])), t["o_ins"]: (250.0, 10.0, np.full(64, tk[t["o_ins"]]))}
    ct = {t["p_ins"]: (300.0, 250.0, np.full(3, trc[t["p_ins"]]))}
    nodes = np.arange(0, len(mesh.coords), 53, dtype=np.int32)
    cond = [[t["p_sample"]], [t["p_coupler"], t["o_coupler"]]]
    out = []
    for tabled in (False, True):
        kw = dict(kappa_tables=kt, rhoc_tables=ct) if tabled else {}
        prob = make_problem(cfg, stack, mesh, precond=1, scheme=scheme, rtol=1e-13, **kw)
        try:
            _, s, ts, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=cond, boundary={2: {3: _heat(cfg).gaussian_dfwhm}},
                                              time_varying=[prob.bcs[3]], **({"tables": {}} if tabled else {}))
            out.append((s, ts, [prob.tangent(j) for j in range(3)]))
        finally:
            prob.close()
    for j in range(3):
        scale = np.max(np.abs(out[0][2][j]))
        err = max(np.max(np.abs(out[0][1][:, j] - out[1][1][:, j])), np.max(np.abs(out[0][2][j] - out[1][2][j]))) / scale
        print(f"{scheme} column {j}: constant tables against the linear run: {err:.2e} of max|s|")
        assert scale > 0 and err <= 1e-9


# 5. error returns ------------------------------------------------------------------------------------------------------------------------
def test_error_returns_and_state_rules(hip, case_with_diamond_small):
    hb = hip
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    tk, trc = material_tables(stack, mesh)
    ins, kt, ct, Tp = _recursion_tables(mesh, tk, trc)
    p_ins, o_ins, sample = ins[0], ins[1], t["p_sample"]
    prob = make_problem(cfg, stack, mesh, precond=1, monitors={"hot": {"tags": [sample], "above": None}})
    be = prob.backend
    try:
        lib, ctx, pi, pd = be._lib, be._ctx, hb._pi, hb._pd
        n_tab = be.tab_len

        def table(entries):
            tab = np.full(n_tab, -1, dtype=np.int32)
            for tag, j in entries.items():
                tab[tag] = j
            return tab

        def err():
            return lib.hf_last_error(ctx).decode()

        def run(n=2):
            g = np.stack([prob.bc_values((k + 1) * prob.dt) for k in range(n)])
            return lib.hf_run_tangent(ctx, n, pd(g), None, 1e-10, 0.0, 1000, 0, None, None, None, None, None)

        def set_tables(kind, entries):
            cols = np.array([c for c, _, _ in entries], dtype=np.int32)
            tags = np.array([tg for _, tg, _ in entries], dtype=np.int32)
            vals = np.ascontiguousarray(np.concatenate([v for _, _, v in entries]), dtype=np.float64)
            return lib.hf_tangent_set_tables(ctx, kind, len(entries), pi(cols), pi(tags), pd(vals))

        def tables_on():
            be.set_kappa_tables(kt)
            be.set_rhoc_tables(ct)
            be.set_state(300.0 * np.ones(prob.n))
            be.assemble(prob.dt, prob.assembly_mode)

        # no tables: the switch needs them
        assert lib.hf_table_derivatives(ctx, 1) == hb.HF_ERR_STATE and "no tables are set" in err()
        tables_on()
        # without the call: the refusals of before, word for word
        assert lib.hf_tangent_setup(ctx, 2, pi(table({sample: 0}))) == hb.HF_ERR_STATE
        assert err() == "hf_tangent_setup: kappa(T) tables are set (tangents of the nonlinear loop are not supported)"
        assert lib.hf_tangent_setup_dir(ctx, 2, pi(table({sample: 0})), None, None) == hb.HF_ERR_STATE
        assert err() == "hf_tangent_setup_dir: kappa(T) tables are set (tangents of the nonlinear loop are not supported)"
        assert run() == hb.HF_ERR_STATE
        assert err() == "hf_run_tangent: kappa(T) tables are set (tangents of the nonlinear loop are not supported)"
        # with it
        assert lib.hf_tangent_set_tables(ctx, 0, 0, None, None, None) == hb.HF_ERR_STATE and "before hf_tangent_setup" in err()
        be.table_derivatives(True)
        assert lib.hf_tangent_setup(ctx, 3, pi(table({p_ins: 0}))) == hb.HF_ERR_ARG
        assert f"tag {p_ins} carries a conductivity table" in err()
        for q in range(3):
            tabs = [None, None, None]
            tabs[q] = pi(table({o_ins: 1}))
            assert lib.hf_tangent_setup_dir(ctx, 3, *tabs) == hb.HF_ERR_ARG and f"tag {o_ins} carries a conductivity table" in err()
        assert lib.hf_tangent_setup(ctx, 3, pi(table({sample: 0}))) == hb.HF_OK
        be.tangent_nv = 4
        assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(table({p_ins: 1}))) == hb.HF_ERR_ARG
        assert f"tag {p_ins} carries a capacity table" in err()
        assert lib.hf_tangent_set_capacity(ctx, n_tab, pi(table({sample: 1}))) == hb.HF_OK      # an untabled tag's capacity is fine
        z = mesh.coords[:, 0]
        assert lib.hf_tangent_set_shape(ctx, 1, pd(np.ascontiguousarray((z - z.min()) / (z.max() - z.min())))) == hb.HF_ERR_STATE
        assert "shape columns under tables" in err()
        # hf_tangent_set_tables: the offenders by name
        good = kt[p_ins][2]
        assert set_tables(0, [(0, sample, good)]) == hb.HF_ERR_ARG and f"tag {sample} carries no conductivity table" in err()
        assert set_tables(1, [(0, t["gasket"], good)]) == hb.HF_ERR_ARG and f"tag {t['gasket']} carries no capacity table" in err()
        for c in (-1, 3, 4):
            assert set_tables(0, [(c, p_ins, good)]) == hb.HF_ERR_ARG and f"column {c} outside [0,3)" in err()
        assert set_tables(0, [(2, p_ins, good), (1, p_ins, good), (2, p_ins, good)]) == hb.HF_ERR_ARG
        assert f"column 2, tag {p_ins} listed twice" in err()
        bad = good.copy()
        bad[4] = np.inf
        assert set_tables(0, [(1, p_ins, good), (2, p_ins, bad)]) == hb.HF_ERR_ARG and f"value 4 of column 2, tag {p_ins} is not finite" in err()
        assert lib.hf_tangent_set_tables(ctx, 2, 0, None, None, None) == hb.HF_ERR_ARG and "kind 2" in err()
        assert lib.hf_tangent_set_tables(ctx, 0, 1, None, None, None) == hb.HF_ERR_ARG
        # a refused call changes nothing; values of either sign are taken; the call resets the tangents
        assert set_tables(0, [(1, p_ins, -good), (1, o_ins, kt[o_ins][2])]) == hb.HF_OK
        assert run(12) == hb.HF_OK and be.get_tangent(1).any() and be.get_tangent(0).any()
        assert set_tables(1, [(2, p_ins, ct[p_ins][2])]) == hb.HF_OK
        assert not any(be.get_tangent(j).any() for j in range(3))
        assert lib.hf_tangent_set_tables(ctx, 0, 0, None, None, None) == hb.HF_OK               # clears the kind
        be.set_state(300.0 * np.ones(prob.n))
        assert run(12) == hb.HF_OK and be.get_tangent(2).any() and be.get_tangent(0).any()
        # more than one Picard sweep, monitor tangents, a source, a batch
        be.set_picard(2)                                                                      # switches the opt-in off ...
        assert run() == hb.HF_ERR_STATE and "tables are set (tangents of the nonlinear loop" in err()
        assert lib.hf_tangent_set_tables(ctx, 0, 0, None, None, None) == hb.HF_ERR_STATE and "table derivatives are off" in err()
        be.table_derivatives(True)                                                            # ... and on again under two sweeps
        assert lib.hf_tangent_setup(ctx, 3, pi(table({sample: 0}))) == hb.HF_OK
        assert run() == hb.HF_ERR_STATE and "2 Picard sweeps" in err()
        be.set_picard(1)
        be.table_derivatives(True)
        assert lib.hf_tangent_setup(ctx, 3, pi(table({sample: 0}))) == hb.HF_OK
        be.set_monitor_tangents(True)
        assert run() == hb.HF_ERR_STATE and "monitor tangents are on" in err()
        be.set_monitor_tangents(False)
        assert run() == hb.HF_OK
        be.set_source([t["p_coupler"]], 1e-5, 0.0)
        assert run() == hb.HF_ERR_STATE and "a source is set" in err()
        be.source_derivatives(True)
        assert run() == hb.HF_ERR_STATE and "a source is set and table derivatives are on" in err()
        assert lib.hf_tangent_setup(ctx, 3, pi(table({sample: 0}))) == hb.HF_ERR_STATE and "a source is set and table derivatives are on" in err()
        assert lib.hf_tangent_set_source(ctx, 0, None) == hb.HF_ERR_STATE and "source columns under tables" in err()
        be.set_source(None)
        assert run() == hb.HF_OK
        # hf_set_kappa_tables switches it off again; so does hf_set_rhoc_tables
        be.set_kappa_tables(kt)
        be.set_state(300.0 * np.ones(prob.n))
        be.assemble(prob.dt, prob.assembly_mode)
        assert run() == hb.HF_ERR_STATE
        assert err() == "hf_run_tangent: kappa(T) tables are set (tangents of the nonlinear loop are not supported)"
        be.table_derivatives(True)
        be.set_rhoc_tables(ct)
        be.set_state(300.0 * np.ones(prob.n))
        be.assemble(prob.dt, prob.assembly_mode)
        assert lib.hf_tangent_setup(ctx, 2, pi(table({sample: 0}))) == hb.HF_ERR_STATE and "tables are set" in err()
        # without tables the linear path is what it was
        be.set_kappa_tables({})
        be.set_rhoc_tables({})
        be.set_state(300.0 * np.ones(prob.n))
        be.assemble(prob.dt, prob.assembly_mode)
        assert lib.hf_tangent_setup(ctx, 2, pi(table({p_ins: 0}))) == hb.HF_OK and run(12) == hb.HF_OK
    finally:
        prob.close()


# 6. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_session_and_fit_of_the_exponent(hip, tmp_path):
    import yaml

    from conftest import load_cfg
    from heatflow_amd.driver import SimulationSession, prepare_mesh
    from heatflow_amd.fit import main, set_params
    from heatflow_amd.geometry import build_stack, scale_mesh_sizes
    from heatflow_amd.parameter_sweep import get_watcher_points

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond_kT"), 8.0)
    cfg["timing"]["num_steps"] = 30
    cfg["timing"]["table_tangents"] = True
    folder = str(tmp_path / "mesh")
    prepare_mesh(cfg, folder, True, build_stack(cfg))
    coords, tris, tags, tag_map = prepare_mesh(cfg, folder, False, build_stack(cfg))      # as the command line will load it
    names = ("p_ins.k", "p_ins.k_power.exponent", "p_sample")
    wp = get_watcher_points(cfg)
    s = SimulationSession(coords, tris, tags, tag_map)
    try:
        res = s.run(cfg, build_stack(cfg), wp, tangents=names)
        assert list(res["tangents"]) == list(names) and res["tangent_iters"].shape == (30, 3)
        for nm in names:
            assert np.max(np.abs(res["tangents"][nm]["oside"])) > 0, nm
        c = set_params(cfg, ("p_ins.k_power.exponent",), (1.1,))       # data made at an exponent of 1.1
        syn = s.run(c, build_stack(c), wp)
        plain = copy.deepcopy(cfg)
        del plain["timing"]["table_tangents"]
        with pytest.raises(ValueError, match=r"tangents does not support temperature-dependent conductivities"):
            s.run(plain, build_stack(plain), wp, tangents=names)
    finally:
        s.close()
    exp_csv = tmp_path / "synthetic.csv"
    np.savetxt(exp_csv, np.column_stack([syn["times"], syn["watchers"]["pside"], syn["watchers"]["oside"]]), delimiter=",",
               header="time,temp,oside", comments="", fmt="%.17g")
    cfg_path, out_dir = tmp_path / "cfg.yaml", tmp_path / "out"
    cfg_path.write_text(yaml.safe_dump(cfg))
    assert main(["--config", str(cfg_path), "--params", "p_ins.k_power.exponent", "--x0", "1.0", "--exp-csv", str(exp_csv),
                 "--mesh-folder", folder, "--output-dir", str(out_dir), "--max-iter", "20"]) == 0
    summary = json.loads((out_dir / "fit_summary.json").read_text())
    print(f"fit of p_ins.k_power.exponent: {summary['values'][0]} (data made at 1.1), off by {summary['values'][0] / 1.1 - 1:.2e}, "
          f"stderr {summary['stderr'][0]:.2e}, {summary['iterations']} iterations, {summary['runs']} runs")
    assert summary["params"] == ["p_ins.k_power.exponent"]
    assert abs(summary["values"][0] / 1.1 - 1) <= 1e-5
    assert np.isfinite(summary["stderr"][0])
    used = yaml.safe_load((out_dir / "used_config.yaml").read_text())
    assert float(used["mats"]["p_ins"]["k_power"]["exponent"]) == pytest.approx(summary["values"][0], rel=1e-12)
    assert used["timing"]["table_tangents"] is True
