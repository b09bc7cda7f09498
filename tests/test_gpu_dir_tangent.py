"""Directional tangents on the GPU (hf_tangent_setup_dir / hf_tangent_load): the load kernel entry by entry
against numpy, its block-stride loop on a lattice of 2054 row blocks, the exact recursion (dir_tangent_oracle.py), finite
differences of GPU primal runs, the Euler identity, the bitwise promises, every error return, and the driver and the fit.

A tag's kappa column and its directional columns do not share a set-up (hf_tangent_setup_dir refuses it: the kernel's table
holds one column per direction and tag), so wherever a list of columns names both for one tag - p_ins.k next to {p_ins, o_ins}.k_z
in the recursion test, p_ins.k next to p_ins.k_r and p_ins.k_z in the Euler identity - the kappa column runs in a second set-up on
the same problem, from the same start, and every column is held to the same bound."""
import json

import numpy as np
import pytest

from aniso_oracle import mixed_multipliers
from conftest import HEATING_CSV, load_cfg
from dir_tangent_oracle import DirTangentOracleBackend, column_weights
from helpers import make_problem

pytestmark = pytest.mark.gpu

NSTEPS = 20


def _heat(cfg):
    from heatflow_amd.heating import HeatingCurve

    return HeatingCurve(HEATING_CSV, float(cfg["heating"]["ic_temp"]), float(cfg["heating"]["fwhm"]))


def element_products(coords, tris, u):
    """Per element and vertex (K_e^r u)_a, (K_e^z u)_a and the same of |K_e| |u|, with the closed form of aniso_oracle.py:
    K^z_ab = |K| rbar b_a b_b / d^2, K^r_ab = |K| rbar c_a c_b / d^2 (b_a = the z-, c_a the r-component of d grad phi_a)."""
    p = np.asarray(coords, dtype=np.float64)[np.asarray(tris, dtype=np.int64)]
    z, r = p[:, :, 0], p[:, :, 1]
    d = (z[:, 1] - z[:, 0]) * (r[:, 2] - r[:, 0]) - (z[:, 2] - z[:, 0]) * (r[:, 1] - r[:, 0])
    b = np.stack([r[:, 1] - r[:, 2], r[:, 2] - r[:, 0], r[:, 0] - r[:, 1]], axis=1)
    c = np.stack([z[:, 2] - z[:, 1], z[:, 0] - z[:, 2], z[:, 1] - z[:, 0]], axis=1)
    ks = (0.5 * np.abs(d) * (r.sum(axis=1) / 3.0) / (d * d))[:, None]
    ue = u[np.asarray(tris, dtype=np.int64)]
    return (ks * c * (c * ue).sum(axis=1)[:, None], ks * b * (b * ue).sum(axis=1)[:, None],
            ks * np.abs(c) * (np.abs(c) * np.abs(ue)).sum(axis=1)[:, None], ks * np.abs(b) * (np.abs(b) * np.abs(ue)).sum(axis=1)[:, None])


def reference_loads(coords, tris, tags, aniso, u, n_cols, k=None, r=None, z=None, products=None):
    """(F, B): F[:, j] = -sum_e w K_e^dir u and B[:, j] = sum_e |w| (|K_e^dir| |u|) per row, element by element in numpy."""
    kr, kz, ar, az = products if products is not None else element_products(coords, tris, u)
    w = column_weights(tags, aniso, n_cols, k, r, z)
    flat, n = np.asarray(tris, dtype=np.int64).ravel(), len(coords)
    F, B = np.zeros((n, n_cols)), np.zeros((n, n_cols))
    for j in range(n_cols):
        if not (w[j] != 0).any():
            continue
        wr, wz = w[j, 0][:, None], w[j, 1][:, None]
        F[:, j] = -np.bincount(flat, weights=(wr * kr + wz * kz).ravel(), minlength=n)
        B[:, j] = np.bincount(flat, weights=(np.abs(wr) * ar + np.abs(wz) * az).ravel(), minlength=n)
    return F, B


def _setups(t):
    """n_par -> (k, r, z) column maps reaching NV = 2, 4, 8, 16: kappa columns on isotropic and anisotropic tags, r and z of one
    tag in two columns, two tags in one column, padded columns (n_par < NV) and, at 9, a column nothing maps to."""
    return {
        2: ({}, {t["p_sample"]: 0}, {t["p_sample"]: 1}),
        3: ({t["p_coupler"]: 0, t["o_coupler"]: 0, t["p_ins"]: 1}, {}, {t["o_ins"]: 2, t["g_ins"]: 2}),
        5: ({t["p_coupler"]: 3, t["gasket"]: 4, t["g_ins"]: 4}, {t["p_sample"]: 0}, {t["p_sample"]: 1, t["p_ins"]: 2, t["o_ins"]: 2}),
        9: ({t["g_ins"]: 6, t["p_coupler"]: 7, t["o_coupler"]: 7}, {t["p_sample"]: 0, t["p_ins"]: 2, t["o_ins"]: 4},
            {t["p_sample"]: 1, t["p_ins"]: 3, t["o_ins"]: 5}),
    }


def _check_loads(be, mesh, aniso, u, n_par, k, r, z, label, zero=(), nonzero=(), products=None):
    nv = next(v for v in (2, 4, 8, 16) if v >= n_par)
    be.tangent_setup_dir(n_par, k, r, z)
    F, B = reference_loads(mesh.coords, mesh.tris, mesh.tags, aniso, u, nv, k, r, z, products)
    worst = 0.0
    for j in range(nv):
        got = be.tangent_load(j)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(B[:, j] > 0, np.abs(got - F[:, j]) / B[:, j], np.where(got == 0, 0.0, np.inf))
        worst = max(worst, float(ratio.max()))
        if j in zero:
            assert np.all(np.abs(got) <= 1e-13 * B[:, j]), (label, n_par, j)
        if j in nonzero:
            assert np.max(np.abs(got) / np.where(B[:, j] > 0, B[:, j], np.inf)) > 1e-6, (label, n_par, j)
        if j >= n_par or not (B[:, j] > 0).any():
            assert np.all(got == 0), (label, n_par, j)
    print(f"{label} n_par={n_par} (NV={nv}): max |F - ref| / sum |K||u| = {worst:.2e}")
    assert worst <= 1e-13, (label, n_par)


def test_loads_entry_by_entry(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    aniso = mixed_multipliers(mesh)
    prob = make_problem(cfg, stack, mesh, k_aniso=aniso, precond=1)
    try:
        be = prob.backend
        prob.run(5, None, time_varying=[prob.bcs[3]])
        u5 = prob.state()
        zc, rc = mesh.coords[:, 0], mesh.coords[:, 1]
        lin_z = 300.0 + 2.0e7 * (zc - zc.min())
        lin_r = 300.0 + 2.0e7 * rc
        for n_par, (k, r, z) in _setups(mesh.material_tags).items():
            rcols, zcols = sorted(set(r.values())), sorted(set(z.values()))
            be.set_state(u5)
            _check_loads(be, mesh, aniso, u5, n_par, k, r, z, "five steps")
            be.set_state(lin_z)       # no radial gradient: every k_r column vanishes, the k_z columns do not
            _check_loads(be, mesh, aniso, lin_z, n_par, k, r, z, "linear in z", zero=rcols, nonzero=zcols)
            be.set_state(lin_r)
            _check_loads(be, mesh, aniso, lin_r, n_par, k, r, z, "linear in r", zero=zcols, nonzero=rcols)
    finally:
        prob.close()


def _jittered_lattice(nz, nr, seed=7):
    """test_gpu_parity._unit_square_mesh(nz, nr) - the mesh of start_vector_oracle.lattice_case - built with array operations, its
    interior nodes jittered as test_gpu_value_lists._lattice jitters them."""
    zs, rs = np.linspace(0.0, 1.0e-6, nz + 1), np.linspace(0.0, 2.0e-6, nr + 1)
    Z, R = np.meshgrid(zs, rs, indexing="ij")
    coords = np.column_stack([Z.ravel(), R.ravel()])
    i, j = (a.ravel() for a in np.meshgrid(np.arange(nz), np.arange(nr), indexing="ij"))
    a, b, c, d = i * (nr + 1) + j, (i + 1) * (nr + 1) + j, (i + 1) * (nr + 1) + j + 1, i * (nr + 1) + j + 1
    tris = np.concatenate([np.column_stack([a, b, c]), np.column_stack([a, c, d])]).astype(np.int32)
    rng = np.random.default_rng(seed)
    inner = (coords[:, 0] > 0) & (coords[:, 0] < 1.0e-6) & (coords[:, 1] > 0) & (coords[:, 1] < 2.0e-6)
    coords[inner, 0] += rng.uniform(-0.3, 0.3, inner.sum()) * 1.0e-6 / nz
    coords[inner, 1] += rng.uniform(-0.3, 0.3, inner.sum()) * 2.0e-6 / nr
    return coords, tris


def test_block_stride_loop_and_partial_last_block(hip):
    """525 625 rows = 2053 x 256 + 57: 2054 row blocks on a grid of 2048 workgroups, six of them in the second pass of the
    block-stride loop, the last with 57 rows.  No solve, no hierarchy."""
    from types import SimpleNamespace

    coords, tris = _jittered_lattice(724, 724)
    n = len(coords)
    assert n == 525625 and (n + 255) // 256 == 2054 and n % 256 == 57
    zc = coords[tris].mean(axis=1)[:, 0]
    tags = (1 + np.minimum((3.0 * zc / 1.0e-6).astype(np.int32), 2)).astype(np.int32)      # three bands in z
    aniso = {1: (2.0, 0.25), 3: (0.5, 3.0)}
    mesh = SimpleNamespace(coords=coords, tris=tris, tags=tags)
    rng = np.random.default_rng(11)
    u = 300.0 + 50.0 * np.sin(3.0e6 * coords[:, 0] + 1.0) * np.cos(1.0e6 * coords[:, 1]) + rng.uniform(-1.0, 1.0, n)
    with hip.HeatflowHIP(0) as be:
        be.set_mesh(coords, tris, tags)
        be.set_materials(np.array([1, 2, 3], dtype=np.int32), np.array([10.0, 3.8, 352.0]), np.array([3.0e6, 2.0e6, 3.4e6]))
        be.set_anisotropy(aniso)
        be.assemble(3e-9, hip.ASM_ROW_GATHER)
        be.set_state(u)
        products = element_products(coords, tris, u)          # once, for both set-ups
        _check_loads(be, mesh, aniso, u, 2, {2: 1}, {1: 0}, {1: 1, 3: 0}, "lattice", products=products)
        _check_loads(be, mesh, aniso, u, 9, {2: 8}, {1: 0, 3: 2}, {1: 1, 3: 3}, "lattice", products=products)


# 3. the exact recursion ---------------------------------------------------------------------------------------------------------
def _recursion_columns(mesh, heat):
    """Two set-ups (see the module text): the issue's columns but p_ins.k, then p_ins.k."""
    t = mesh.material_tags
    first = ([[(t["p_sample"], "r")], [(t["p_sample"], "z")], [(t["p_ins"], "z"), (t["o_ins"], "z")], [t["p_coupler"]], []],
             {4: {3: heat.gaussian_dfwhm}}, ["p_sample.k_r", "p_sample.k_z", "{p_ins,o_ins}.k_z", "p_coupler", "fwhm"])
    second = ([[(t["p_ins"], "k")]], {}, ["p_ins.k"])
    return first, second


def _recursion_run(prob, mesh, heat, nodes, ic):
    """[(name, samples (n_steps, n_s), final field)] of every column, the two set-ups run one after the other from the start."""
    out = []
    for cond, bnd, names in _recursion_columns(mesh, heat):
        prob.set_state(ic)
        _, _, ts, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=cond, boundary=bnd, time_varying=[prob.bcs[3]])
        out += [(nm, ts[:, j], prob.tangent(j)) for j, nm in enumerate(names)]
    return out


@pytest.mark.parametrize("scheme", ["backward_euler", "bdf2"])
@pytest.mark.parametrize("case", ["case_with_diamond_small", "case_no_diamond_small"])
def test_tangents_match_the_exact_recursion(hip, request, case, scheme):
    cfg, stack, mesh = request.getfixturevalue(case)
    heat, ic = _heat(cfg), float(cfg["heating"]["ic_temp"])
    aniso = mixed_multipliers(mesh)
    nodes = np.sort(np.random.default_rng(0).choice(len(mesh.coords), 12, replace=False)).astype(np.int32)
    ref = _recursion_run(make_problem(cfg, stack, mesh, backend=DirTangentOracleBackend(), k_aniso=aniso, scheme=scheme),
                         mesh, heat, nodes, ic)
    for precond in (0, 1):
        prob = make_problem(cfg, stack, mesh, precond=precond, k_aniso=aniso, scheme=scheme)
        try:
            got = _recursion_run(prob, mesh, heat, nodes, ic)
        finally:
            prob.close()
        for (nm, ts, field), (_, ts_ref, field_ref) in zip(got, ref):
            scale = np.max(np.abs(field_ref))
            assert scale > 0
            err_s, err_f = np.max(np.abs(ts - ts_ref)) / scale, np.max(np.abs(field - field_ref)) / scale
            print(f"{case} {scheme} precond={precond} {nm}: samples off by {err_s:.2e}, final field by {err_f:.2e} of max|s|")
            assert err_s <= 1e-6 and err_f <= 1e-6, (case, scheme, precond, nm)


# 4. finite differences of GPU primal runs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p_sample.k_r", "p_sample.k_z", "p_ins.k_r", "p_ins.k_z"])
def test_tangents_match_finite_differences_of_gpu_runs(hip, case_with_diamond_small, name):
    """The fourth-order central quotient of primal runs at the multiplier m (1 +- h), m (1 +- 2h), h = 1e-2, divided by h m k,
    with multigrid at rtol = 1e-12 over 40 steps; bound 1e-6 of max |s|.  On the restatement (sparse LU; test_dir_tangent_cpu.py)
    the quotient's truncation error is at most 1.5e-8 of max |s|, the second-order quotient's 1e-5 .. 5e-5; an error eps of the
    primal runs enters as 1.5 eps / (h max|s| k_dir)."""
    cfg, stack, mesh = case_with_diamond_small
    aniso = mixed_multipliers(mesh)
    mat, suffix = name.rsplit(".", 1)
    tag, q = mesh.material_tags[mat], 0 if suffix == "k_r" else 1
    nsteps, h = 40, 1e-2
    nodes = np.arange(0, len(mesh.coords), max(1, len(mesh.coords) // 50), dtype=np.int32)
    prob = make_problem(cfg, stack, mesh, precond=1, rtol=1e-12, k_aniso=aniso)
    try:
        _, _, ts, _, _ = prob.run_tangent(nsteps, nodes, conductivity=[[(tag, "rz"[q])]], time_varying=[prob.bcs[3]])
    finally:
        prob.close()
    runs = {}
    for f in (2, 1, -1, -2):
        a = dict(aniso)
        m = list(a[tag])
        m[q] *= 1.0 + f * h
        a[tag] = tuple(m)
        p = make_problem(cfg, stack, mesh, precond=1, rtol=1e-12, k_aniso=a)
        try:
            runs[f] = p.run(nsteps, nodes, time_varying=[p.bcs[3]])[1]
        finally:
            p.close()
    k_dir = float(cfg["mats"][mat]["k"]) * aniso[tag][q]
    fd2 = (runs[1] - runs[-1]) / (2.0 * h * k_dir)
    fd4 = (8.0 * (runs[1] - runs[-1]) - (runs[2] - runs[-2])) / (12.0 * h * k_dir)
    scale = float(np.max(np.abs(ts[:, 0])))
    assert scale > 0
    e2, e4 = float(np.max(np.abs(ts[:, 0] - fd2))), float(np.max(np.abs(ts[:, 0] - fd4)))
    print(f"{name}: max |s| k_dir = {scale * k_dir:.3e} K; |s - FD2| / max|s| = {e2 / scale:.2e}, |s - FD4| / max|s| = {e4 / scale:.2e}")
    assert e4 <= 1e-6 * scale


# 5. the Euler identity -------------------------------------------------------------------------------------------------------------
def test_euler_identity_on_the_device(hip, case_with_diamond_small):
    """s_kappa = m_r s_kr + m_z s_kz for p_ins, within the sum of the three columns' bounds against the recursion."""
    cfg, stack, mesh = case_with_diamond_small
    aniso = mixed_multipliers(mesh)
    tag = mesh.material_tags["p_ins"]
    m_r, m_z = aniso[tag]
    nodes = np.arange(0, len(mesh.coords), 53, dtype=np.int32)
    prob = make_problem(cfg, stack, mesh, precond=1, k_aniso=aniso)
    try:
        _, _, tk, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=[[(tag, "k")]], time_varying=[prob.bcs[3]])
        sk_field = prob.tangent(0)
        prob.set_state(float(cfg["heating"]["ic_temp"]))
        _, _, td, _, _ = prob.run_tangent(NSTEPS, nodes, conductivity=[[(tag, "r")], [(tag, "z")]], time_varying=[prob.bcs[3]])
        sr_field, sz_field = prob.tangent(0), prob.tangent(1)
    finally:
        prob.close()
    for what, sk, sr, sz in (("samples", tk[:, 0], td[:, 0], td[:, 1]), ("final field", sk_field, sr_field, sz_field)):
        err = np.max(np.abs(sk - (m_r * sr + m_z * sz)))
        bound = 1e-6 * (np.max(np.abs(sk)) + m_r * np.max(np.abs(sr)) + m_z * np.max(np.abs(sz)))
        print(f"Euler identity, {what}: |s_k - (m_r s_kr + m_z s_kz)| = {err:.2e}, bound {bound:.2e}")
        assert np.max(np.abs(sk)) > 0 and err <= bound


# 6. bit for bit ----------------------------------------------------------------------------------------------------------------------
def test_primal_under_a_directional_set_up_is_bitwise_that_of_hf_run(hip, case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    aniso = mixed_multipliers(mesh)
    t = mesh.material_tags
    nodes = np.arange(0, len(mesh.coords), 97, dtype=np.int32)
    cond = [[(t["p_sample"], "r")], [(t["p_sample"], "z"), (t["p_ins"], "z")], [(t["g_ins"], "k")]]
    for precond in (0, 1):
        out = []
        for tangent in (False, True):
            prob = make_problem(cfg, stack, mesh, precond=precond, k_aniso=aniso)
            try:
                if tangent:
                    _, s1, _, it1, _ = prob.run_tangent(12, nodes, conductivity=cond, time_varying=[prob.bcs[3]])
                    _, s2, _, it2, _ = prob.run_tangent(6, nodes, conductivity=cond, time_varying=[prob.bcs[3]], first_step=12)
                else:
                    _, s1, it1 = prob.run(12, nodes, time_varying=[prob.bcs[3]])
                    _, s2, it2 = prob.run(6, nodes, time_varying=[prob.bcs[3]], first_step=12)
                out.append((s1, it1, s2, it2, prob.state()))
            finally:
                prob.close()
        for a, b in zip(*out):
            assert np.array_equal(a, b), precond


@pytest.mark.parametrize("listed", [False, True])
def test_kappa_columns_at_unit_multipliers_give_the_bits_of_hf_tangent_setup(hip, case_with_diamond_small, listed):
    """No anisotropy (or every multiplier listed as (1, 1)): a directional set-up of kappa columns gives the loads and the
    tangent samples of hf_tangent_setup with the same columns, bit for bit."""
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    groups = [[t["p_sample"]], [t["p_coupler"], t["o_coupler"]], [t["p_ins"]]]
    nodes = np.arange(0, len(mesh.coords), 53, dtype=np.int32)
    kw = {"k_aniso": {t["p_sample"]: (1.0, 1.0), t["p_ins"]: (1.0, 1.0)}} if listed else {}
    out = []
    for directional in (False, True):
        prob = make_problem(cfg, stack, mesh, precond=1, **kw)
        try:
            cond = [[(tag, "k") for tag in g] for g in groups] if directional else groups
            _, s, ts, it, tit = prob.run_tangent(NSTEPS, nodes, conductivity=cond, time_varying=[prob.bcs[3]])
            loads = [prob.tangent_load(j) for j in range(4)]
            out.append([s, ts, it, tit, prob.state()] + loads + [prob.tangent(j) for j in range(3)])
        finally:
            prob.close()
    assert np.max(np.abs(out[0][5])) > 0 and np.max(np.abs(out[0][1])) > 0
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# 7. errors and staleness -------------------------------------------------------------------------------------------------------------
def test_error_returns_and_staleness(hip, case_with_diamond_small):
    hb = hip
    cfg, stack, mesh = case_with_diamond_small
    t = mesh.material_tags
    aniso = mixed_multipliers(mesh)
    t_an, t_iso = t["p_sample"], t["p_coupler"]
    prob = make_problem(cfg, stack, mesh, k_aniso=aniso)
    be = prob.backend
    try:
        lib, ctx, pi, pd = be._lib, be._ctx, hb._pi, hb._pd
        g = np.stack([prob.bc_values((k + 1) * prob.dt) for k in range(2)])
        none = np.full(be.tab_len, -1, dtype=np.int32)
        buf = np.zeros(prob.n)

        def tab(cols):
            a = none.copy()
            for tag, j in cols.items():
                a[tag] = j
            return a

        def err():
            return lib.hf_last_error(ctx).decode()

        def run():
            return lib.hf_run_tangent(ctx, 2, pd(g), None, 1e-10, 0.0, 1000, 0, None, None, None, None, None)

        assert lib.hf_tangent_load(ctx, 0, pd(buf)) == hb.HF_ERR_STATE and "hf_tangent_load before" in err()
        # bad arguments, each naming the tag where there is one
        for n_par in (0, 17):
            assert lib.hf_tangent_setup_dir(ctx, n_par, pi(none), None, None) == hb.HF_ERR_ARG and "1..16 parameters" in err()
        assert lib.hf_tangent_setup_dir(ctx, 2, None, None, None) == hb.HF_ERR_ARG and "all null" in err()
        for which in range(3):
            for bad in (2, -2):
                tabs = [None, None, None]
                tabs[which] = pi(tab({t_an: bad}))
                assert lib.hf_tangent_setup_dir(ctx, 2, *tabs) == hb.HF_ERR_ARG
                assert f"tag {t_an} " in err() and "outside [-1,2)" in err()
        for unused in sorted(set(range(be.tab_len)) - set(mesh.tags.tolist()))[:1]:
            assert lib.hf_tangent_setup_dir(ctx, 1, None, pi(tab({unused: 0})), None) == hb.HF_ERR_ARG
            assert f"tag {unused} is not a cell tag" in err()
        for other in (1, 2):
            tabs = [pi(tab({t_an: 0})), None, None]
            tabs[other] = pi(tab({t_an: 1}))
            assert lib.hf_tangent_setup_dir(ctx, 2, *tabs) == hb.HF_ERR_ARG
            assert f"tag {t_an} has a kappa column and a directional one" in err()
        assert lib.hf_tangent_load(ctx, 0, pd(buf)) == hb.HF_ERR_STATE          # the refused calls left no set-up
        # a good set-up; hf_tangent_load's arguments
        assert lib.hf_tangent_setup_dir(ctx, 2, None, pi(tab({t_an: 0})), pi(tab({t_an: 1}))) == hb.HF_OK
        assert lib.hf_tangent_load(ctx, 0, pd(buf)) == hb.HF_OK
        for j in (-1, 2):
            assert lib.hf_tangent_load(ctx, j, pd(buf)) == hb.HF_ERR_ARG and "outside [0,2)" in err()
        assert run() == hb.HF_OK
        # state errors: a batch open, a load set
        be.batch_begin(2, 0)
        assert lib.hf_tangent_setup_dir(ctx, 1, pi(tab({t_an: 0})), None, None) == hb.HF_ERR_STATE and "a batch is open" in err()
        assert lib.hf_tangent_load(ctx, 0, pd(buf)) == hb.HF_ERR_STATE and "a batch is open" in err()
        assert run() == hb.HF_ERR_STATE
        be.batch_end()
        be.set_load(np.zeros(prob.n))
        assert lib.hf_tangent_setup_dir(ctx, 1, pi(tab({t_an: 0})), None, None) == hb.HF_ERR_STATE and "a load is set" in err()
        assert run() == hb.HF_ERR_STATE
        be.set_load(None)
        assert run() == hb.HF_OK
        # the steady-state lock of hf_run_tangent holds for this set-up too
        be.steady_setup(prob.bc_dofs)
        be.steady_solve(prob.bc_values(0.0))
        assert run() == hb.HF_ERR_STATE and "hf_steady_solve" in err()
        assert lib.hf_tangent_setup_dir(ctx, 1, pi(tab({t_an: 0})), None, None) == hb.HF_OK
        assert run() == hb.HF_ERR_STATE
        be.set_state(np.full(prob.n, 300.0))
        assert run() == hb.HF_OK
        # hf_tangent_setup on an anisotropic tag is still refused after a directional set-up existed, and replaces nothing
        with pytest.raises(ValueError, match=f"hf_tangent_setup: tag {t_an} is anisotropic"):
            be.tangent_setup(1, {t_an: 0})
        assert run() == hb.HF_OK
        # stale after hf_set_materials (until hf_assemble) ...
        tags = sorted(t.values())
        tk = {t[m.name]: m.properties["k"] for m in stack.materials}
        trc = {t[m.name]: m.properties["rho_cv"] for m in stack.materials}
        be.set_materials(np.array(tags, dtype=np.int32), np.array([tk[v] for v in tags]), np.array([trc[v] for v in tags]))
        assert run() == hb.HF_ERR_STATE and "before hf_assemble" in err()
        be.assemble(prob.dt, hb.ASM_ROW_GATHER)
        assert run() == hb.HF_OK
        # ... and gone after hf_set_anisotropy: its kappa weights were the old multipliers
        be.set_anisotropy({t_an: (4.0, 0.5)})
        assert run() == hb.HF_ERR_STATE and "before hf_tangent_setup" in err()
        assert lib.hf_tangent_load(ctx, 0, pd(buf)) == hb.HF_ERR_STATE
        be.assemble(prob.dt, hb.ASM_ROW_GATHER)
        assert lib.hf_get_tangent(ctx, 0, pd(buf)) == hb.HF_ERR_STATE
        # tables set: refused (after the multipliers are cleared, which the tables need)
        be.set_anisotropy({})
        be.set_kappa_tables({t_iso: (300.0, 10.0, [1.0, 2.0])})
        assert lib.hf_tangent_setup_dir(ctx, 1, pi(tab({t_an: 0})), None, None) == hb.HF_ERR_STATE and "tables are set" in err()
        be.set_kappa_tables({})
        # an assembly in another mode: the set-up made before is stale, a new one is refused
        be.assemble(prob.dt, hb.ASM_ROW_GATHER)
        be.set_state(np.full(prob.n, 300.0))
        assert lib.hf_tangent_setup_dir(ctx, 1, None, None, pi(tab({t_an: 0}))) == hb.HF_OK
        assert run() == hb.HF_OK
        be.assemble(prob.dt, hb.ASM_LDS_COLORED)
        assert run() == hb.HF_ERR_ARG and "row-gather" in err()
        assert lib.hf_tangent_setup_dir(ctx, 1, None, None, pi(tab({t_an: 0}))) == hb.HF_ERR_ARG and "row-gather" in err()
        # hf_set_mesh removes it
        be.set_mesh(mesh.coords, mesh.tris, mesh.tags)
        assert lib.hf_tangent_load(ctx, 0, pd(buf)) == hb.HF_ERR_STATE
        assert run() == hb.HF_ERR_STATE
    finally:
        prob.close()
    # a tag value below the largest that no cell carries: a mesh of two triangles with tags 0 and 2
    be = hip.HeatflowHIP()
    try:
        be.set_mesh(np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), np.array([[0, 1, 2], [0, 2, 3]]), np.array([0, 2]))
        for which in range(3):
            tabs = [None, None, None]
            tabs[which] = hip._pi(np.array([-1, 0, -1], dtype=np.int32))
            assert be._lib.hf_tangent_setup_dir(be._ctx, 1, *tabs) == hip.HF_ERR_ARG
            assert "tag 1 is not a cell tag" in be._lib.hf_last_error(be._ctx).decode()
    finally:
        be.close()


# 8. driver and fit -------------------------------------------------------------------------------------------------------------------
def test_session_and_fit_of_k_z_of_the_sample(hip, tmp_path):
    import yaml

    from heatflow_amd.driver import SimulationSession, prepare_mesh
    from heatflow_amd.fit import get_param, main, set_params
    from heatflow_amd.geometry import build_stack, scale_mesh_sizes
    from heatflow_amd.parameter_sweep import get_watcher_points

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond_aniso"), 8.0)
    cfg["timing"]["num_steps"] = 30
    folder = str(tmp_path / "mesh")
    mesh = prepare_mesh(cfg, folder, True, build_stack(cfg))
    names = ["p_sample.k_z", "p_ins.k_r", "fwhm"]
    k0 = get_param(cfg, "p_sample.k_z")
    s = SimulationSession(*mesh)
    try:
        res = s.run(cfg, build_stack(cfg), get_watcher_points(cfg), tangents=names)
        assert list(res["tangents"]) == names and res["tangent_iters"].shape == (30, 3)
        for nm in names:
            assert set(res["tangents"][nm]) == set(res["watcher_names"]) == {"pside", "oside"}
            assert np.max(np.abs(res["tangents"][nm]["oside"])) > 0
        c = set_params(cfg, ("p_sample.k_z",), (1.2 * k0,))
        syn = s.run(c, build_stack(c), get_watcher_points(c))
    finally:
        s.close()
    exp_csv = tmp_path / "synthetic.csv"
    np.savetxt(exp_csv, np.column_stack([syn["times"], syn["watchers"]["pside"], syn["watchers"]["oside"]]), delimiter=",",
               header="time,temp,oside", comments="", fmt="%.17g")
    cfg_path, out_dir = tmp_path / "cfg.yaml", tmp_path / "out"
    cfg_path.write_text(yaml.safe_dump(cfg))
    assert main(["--config", str(cfg_path), "--params", "p_sample.k_z", "--x0", repr(k0), "--exp-csv", str(exp_csv),
                 "--mesh-folder", folder, "--output-dir", str(out_dir), "--max-iter", "20"]) == 0
    summary = json.loads((out_dir / "fit_summary.json").read_text())
    print(f"fit of p_sample.k_z: {summary['values'][0]} (data made at {1.2 * k0}), stderr {summary['stderr'][0]:.2e}, "
          f"{summary['iterations']} iterations, {summary['runs']} runs")
    assert summary["params"] == ["p_sample.k_z"]
    assert abs(summary["values"][0] / (1.2 * k0) - 1) <= 1e-5
    assert np.isfinite(summary["stderr"][0])
    used = yaml.safe_load((out_dir / "used_config.yaml").read_text())
    k = float(cfg["mats"]["p_sample"]["k"])
    assert used["mats"]["p_sample"]["k_aniso"]["z"] == pytest.approx(summary["values"][0] / k, rel=1e-12)
    assert used["mats"]["p_ins"]["k_aniso"] == {"r": 2.0, "z": 0.25} and used["mats"]["p_sample"]["k"] == k
