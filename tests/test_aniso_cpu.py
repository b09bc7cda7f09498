"""Anisotropic conductivities without a GPU: the restatement of tests/aniso_oracle.py (against the isotropic loop, a quadrature
of the weak form, the stretch identity and two one-dimensional problems that separate the directions), the configuration key,
used_config.yaml, HeatProblem's call order, every Python refusal, and the header."""
import copy
import os
import re

import numpy as np
import pytest

from aniso_oracle import (BDF2, BE, aniso_fields, element_matrices_aniso, element_matrices_aniso_quadrature,
                          matrices, mixed_multipliers, operator, steady_solve, stretched)
from conftest import ROOT, build_case, load_cfg
from kappa_T_oracle import linear_fields, problem_inputs
from oracle import heat_oracle as ho

STRETCH_ENTRY_TOL = 1e-13      # of |M_ij| + dt |K_ij|
STRETCH_FIELD_TOL_K = 1e-9


@pytest.fixture(scope="module")
def small():
    return build_case("geballe_with_diamond", 8.0)


@pytest.fixture(scope="module")
def small_nd():
    return build_case("geballe_no_diamond", 8.0)


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", [BE, BDF2])
def test_unit_multipliers_equal_the_linear_oracle_bit_for_bit(small, scheme):
    cfg, stack, mesh = small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 20)
    lin = linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, scheme)
    for aniso in ({}, {t: (1.0, 1.0) for t in tk}):
        an = aniso_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, aniso, scheme)
        assert np.array_equal(an, lin)
    assert np.abs(lin[-1] - lin[0]).max() > 1.0


def test_equal_multipliers_are_a_scaled_isotropic_conductivity_bit_for_bit(small):
    cfg, stack, mesh = small
    tk, trc, *_ = problem_inputs(cfg, stack, mesh, 1)
    t = mesh.material_tags["p_ins"]
    M, K = matrices(mesh.coords, mesh.tris, mesh.tags, tk, trc, {t: (3.0, 3.0)})
    M0, K0 = matrices(mesh.coords, mesh.tris, mesh.tags, {**tk, t: tk[t] * 3.0}, trc, {})
    assert np.array_equal(M.data, M0.data) and np.array_equal(K.data, K0.data)


def test_closed_form_matches_a_quadrature_of_the_weak_form():
    rng = np.random.default_rng(11)
    zr = rng.random((60, 2)) + np.array([0.0, 0.2])
    tri = np.array([rng.choice(60, 3, replace=False) for _ in range(200)])
    rho_c, kappa = 1.0 + rng.random(200), 1.0 + rng.random(200)
    m_r, m_z = 0.25 + 4.0 * rng.random(200), 0.25 + 4.0 * rng.random(200)
    Me, Ke = element_matrices_aniso(zr, tri, rho_c, kappa, m_r, m_z)
    Mq, Kq = element_matrices_aniso_quadrature(zr, tri, rho_c, kappa, m_r, m_z)
    assert np.abs(Me - Mq).max() <= 1e-12 * np.abs(Mq).max()
    assert np.abs(Ke - Kq).max() <= 1e-12 * np.abs(Kq).max()
    # the quadrature sees which direction a multiplier belongs to: swapping them is another matrix
    _, Ks = element_matrices_aniso(zr, tri, rho_c, kappa, m_z, m_r)
    assert np.abs(Ks - Kq).max() > 1e-2 * np.abs(Kq).max()
    # rows of K sum to zero (constants are in the kernel of the stiffness) and K is symmetric
    assert np.abs(Ke.sum(axis=2)).max() <= 1e-12 * np.abs(Ke).max()
    assert np.array_equal(Ke, Ke.transpose(0, 2, 1))


@pytest.mark.parametrize("which", ["small", "small_nd"])
def test_stretch_identity(request, which):
    """One ratio k_r / k_z = s^2 for every material = the isotropic problem k / s, rho_c / s on (s z, r), matrix for matrix."""
    cfg, stack, mesh = request.getfixturevalue(which)
    nsteps = 20
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, nsteps)
    s = 2.0
    aniso = {t: (1.0, 1.0 / (s * s)) for t in tk}
    M, A, K = operator(mesh.coords, mesh.tris, mesh.tags, tk, trc, aniso, dt)
    cs, ks, rcs = stretched(mesh.coords, tk, trc, s)
    Ms, As, Ks = operator(cs, mesh.tris, mesh.tags, ks, rcs, {}, dt)
    scale = abs(M) + dt * abs(K)
    for X, Xs in ((M, Ms), (A, As), (dt * K, dt * Ks)):
        D = abs(X - Xs).tocsr()
        worst = (D.data / np.asarray(scale[D.nonzero()]).ravel()).max() if D.nnz else 0.0
        print(f"{which}: worst entry difference / (|M| + dt |K|) = {worst:.2e}")
        assert worst <= STRETCH_ENTRY_TOL
    f = aniso_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, aniso)
    fs = linear_fields(cs, mesh.tris, mesh.tags, ks, rcs, dt, dofs, u0, g)
    iso = linear_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g)
    worst = np.abs(f - fs).max()
    print(f"{which}: fields differ by {worst:.2e} K; the anisotropy moves the field by {np.abs(f - iso).max():.1f} K")
    assert worst <= STRETCH_FIELD_TOL_K
    assert np.abs(f - iso).max() > 10.0
    # the mixed case of the GPU tests moves the field as far, with A exactly symmetric
    mixed = mixed_multipliers(mesh)
    fm = aniso_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, mixed)
    assert np.abs(fm - iso).max() > 10.0
    _, Am, _ = operator(mesh.coords, mesh.tris, mesh.tags, tk, trc, mixed, dt)
    assert abs(Am - Am.T).max() <= 1e-20


# ---- two one-dimensional problems that separate the directions --------------------------------------------------------------
def _grid(z, r, tag_of):
    """Structured triangulation of the grid z x r (every rectangle split by the same diagonal); tag_of(zc, rc) per triangle."""
    nz, nr = len(z), len(r)
    zz, rr = np.meshgrid(z, r, indexing="ij")
    coords = np.column_stack([zz.ravel(), rr.ravel()])
    idx = lambda i, j: i * nr + j
    tris = []
    for i in range(nz - 1):
        for j in range(nr - 1):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            tris += [[a, b, c], [a, c, d]]
    tris = np.array(tris)
    cen = coords[tris].mean(axis=1)
    tags = np.array([tag_of(zc, rc) for zc, rc in cen], dtype=np.int32)
    return coords, tris, tags


def test_layered_slab_follows_the_series_resistance_in_m_z_k_and_ignores_m_r():
    """Two layers stacked along z between held faces: the steady field is piecewise linear in z - a member of the P1 space, so the
    Galerkin solution is exact - with the interface temperature of two resistances h_i / (m_z,i k_i) in series; the radial
    conductivities never enter."""
    z = np.linspace(0.0, 4e-6, 9)
    r = np.linspace(0.0, 3e-6, 7)
    coords, tris, tags = _grid(z, r, lambda zc, rc: 1 if zc < 2e-6 else 2)
    tk, trc = {1: 10.0, 2: 3.0}, {1: 1.0, 2: 1.0}
    lo, hi = np.nonzero(coords[:, 0] == z[0])[0], np.nonzero(coords[:, 0] == z[-1])[0]
    dofs = np.concatenate([lo, hi])
    g = np.concatenate([np.full(len(lo), 300.0), np.full(len(hi), 400.0)])
    mid = np.nonzero(coords[:, 0] == 2e-6)[0]
    out = {}
    for m_r in (1.0, 7.0):
        for mz1, mz2 in ((1.0, 1.0), (0.25, 1.0), (0.25, 4.0)):
            _, K = matrices(coords, tris, tags, tk, trc, {1: (m_r, mz1), 2: (1.0 / m_r, mz2)})
            u = steady_solve(K, dofs, g)
            R1, R2 = 2e-6 / (mz1 * tk[1]), 2e-6 / (mz2 * tk[2])
            t_int = 300.0 + 100.0 * R1 / (R1 + R2)
            assert np.abs(u[mid] - t_int).max() <= 1e-9, (m_r, mz1, mz2)
            exact = np.where(coords[:, 0] <= 2e-6, 300.0 + (t_int - 300.0) * coords[:, 0] / 2e-6,
                             t_int + (400.0 - t_int) * (coords[:, 0] - 2e-6) / 2e-6)
            assert np.abs(u - exact).max() <= 1e-9
            out[(m_r, mz1, mz2)] = u
    for key in ((1.0, 1.0), (0.25, 1.0), (0.25, 4.0)):
        assert np.abs(out[(1.0,) + key] - out[(7.0,) + key]).max() <= 1e-9        # m_r does not move it
    assert np.abs(out[(1.0, 1.0, 1.0)] - out[(1.0, 0.25, 1.0)]).max() > 10.0     # m_z does


def test_field_between_two_radii_ignores_m_z():
    """Two shells between held radii a < c < b: the steady field is piecewise logarithmic in r with the interface temperature of
    the radial resistances ln(r_out / r_in) / (m_r k); the axial conductivities never enter.
    On the matrix level that is exact: a nodal field that depends on r alone has no z-gradient on any triangle of the grid, so
    K(m_z) u = K(m_z') u to rounding.  On the solution level the discrete field is not exactly a function of r (the end columns
    of the grid see half supports), so two m_z agree to the discretisation error only: the bound is the P1 interpolation error
    h_r^2 / 8 max |u''| of the logarithm, times 4 for the two solutions and the Galerkin constant."""
    a, c, b = 1e-6, 2e-6, 4e-6
    r = np.concatenate([np.linspace(a, c, 33), np.linspace(c, b, 65)[1:]])
    z = np.linspace(0.0, 1e-6, 5)
    coords, tris, tags = _grid(z, r, lambda zc, rc: 1 if rc < c else 2)
    tk, trc = {1: 10.0, 2: 3.0}, {1: 1.0, 2: 1.0}
    m_r = {1: 2.0, 2: 0.5}
    inner, outer = np.nonzero(coords[:, 1] == a)[0], np.nonzero(coords[:, 1] == b)[0]
    dofs = np.concatenate([inner, outer])
    g = np.concatenate([np.full(len(inner), 400.0), np.full(len(outer), 300.0)])

    def interface(kr1, kr2):
        R1, R2 = np.log(c / a) / kr1, np.log(b / c) / kr2
        return 400.0 - 100.0 * R1 / (R1 + R2)

    t_int = interface(m_r[1] * tk[1], m_r[2] * tk[2])
    rr = coords[:, 1]
    exact = np.where(rr <= c, 400.0 + (t_int - 400.0) * np.log(rr / a) / np.log(c / a),
                     t_int + (300.0 - t_int) * np.log(rr / c) / np.log(b / c))
    h = np.diff(r).max()
    upp = max((400.0 - t_int) / (a * a * np.log(c / a)), (t_int - 300.0) / (c * c * np.log(b / c)))
    tol = 4.0 * h * h / 8.0 * upp
    assert tol < 0.05
    # matrix level, exact
    rng = np.random.default_rng(5)
    u_r = (300.0 + 100.0 * rng.random(len(r)))[np.searchsorted(r, rr)]
    Ks = {}
    for mz in (1.0, 1.0 / 16.0, 16.0):
        _, K = matrices(coords, tris, tags, tk, trc, {1: (m_r[1], mz), 2: (m_r[2], 1.0 / mz)})
        Ks[mz] = K
    for mz in (1.0 / 16.0, 16.0):
        assert np.all(np.abs(Ks[mz] @ u_r - Ks[1.0] @ u_r) <= 1e-13 * (abs(Ks[1.0]) @ np.abs(u_r)))
        assert abs(Ks[mz] - Ks[1.0]).max() > 1e-3 * abs(Ks[1.0]).max()           # (the matrices themselves differ)
    # solution level
    sol = {mz: steady_solve(K, dofs, g) for mz, K in Ks.items()}
    for mz, u in sol.items():
        print(f"m_z = {mz}: max |u - exact| = {np.abs(u - exact).max():.2e} K (bound {tol:.2e})")
        assert np.abs(u - exact).max() <= tol
        assert np.abs(u - sol[1.0]).max() <= tol
    # a kernel that gave m_z to the radial direction would move the interface by far more than the bound
    assert abs(interface(tk[1] / 16.0, tk[2] * 16.0) - t_int) > 100.0 * tol


# ---- configuration ---------------------------------------------------------------------------------------------------------
def test_config_key_is_parsed_into_the_stack():
    from heatflow_amd.aniso import aniso_keys, material_aniso
    from heatflow_amd.geometry import build_stack

    cfg = load_cfg("geballe_with_diamond_aniso")
    stack = build_stack(cfg)
    an = {m.name: m.properties["k_aniso"] for m in stack.materials if "k_aniso" in m.properties}
    assert an == {"p_ins": (2.0, 0.25), "o_ins": (2.0, 0.25), "g_ins": (2.0, 0.25)}
    assert aniso_keys(cfg) == ["mats.g_ins.k_aniso", "mats.o_ins.k_aniso", "mats.p_ins.k_aniso"]
    assert stack.by_name("p_ins").properties["k"] == 10.0                       # k itself stays
    assert all("k_aniso" not in m.properties for m in build_stack(load_cfg("geballe_with_diamond")).materials)
    assert material_aniso("x", {"k": 1.0}) is None
    assert material_aniso("x", {"k_aniso": {"r": 2}}) == (2.0, 1.0)             # either key may be absent
    assert material_aniso("x", {"k_aniso": {"z": "5e-1"}}) == (1.0, 0.5)
    assert material_aniso("x", {"k_aniso": {}}) == (1.0, 1.0)
    for bad in ({"r": 0.0}, {"z": -1.0}, {"r": float("nan")}, {"r": float("inf")}, {"r": 2.0, "phi": 1.0}, {"r": "two"}, [2.0, 0.25],
                3.0):
        c = copy.deepcopy(load_cfg("geballe_with_diamond"))
        c["mats"]["p_sample"]["k_aniso"] = bad
        with pytest.raises(ValueError, match=r"mats\.p_sample\.k_aniso"):
            build_stack(c)


@pytest.mark.parametrize("key,block", [("k_table", {"T_min": 300.0, "T_max": 700.0, "k": [4.0, 3.0]}),
                                       ("k_power", {"T_ref": 300.0, "exponent": 1.0, "T_min": 300.0, "T_max": 900.0}),
                                       ("cv_table", {"T_min": 300.0, "T_max": 700.0, "cv": [600.0, 700.0]}),
                                       ("cv_einstein", {"theta": 600.0, "T_ref": 300.0, "T_min": 300.0, "T_max": 900.0})])
def test_k_aniso_with_a_table_key_is_refused_naming_both(key, block):
    from heatflow_amd.geometry import build_stack

    c = copy.deepcopy(load_cfg("geballe_with_diamond_aniso"))
    c["mats"]["o_diam"][key] = block                                             # on another material: still one configuration
    with pytest.raises(ValueError, match=rf"mats\.g_ins\.k_aniso.*mats\.o_diam\.{key}"):
        build_stack(c)


@pytest.mark.parametrize("key,block", [("k_table", {"T_min": 300.0, "T_max": 700.0, "k": [4.0, 3.0]}),
                                       ("cv_einstein", {"theta": 600.0, "T_ref": 300.0, "T_min": 300.0, "T_max": 900.0})])
def test_the_drivers_refuse_k_aniso_with_a_table_key_before_any_mesh_or_session(key, block, tmp_path):
    from heatflow_amd.driver import run_simulation_batch_impl, run_simulation_impl

    class Untouched:                                                             # any use of the session is an AttributeError
        pass

    c = copy.deepcopy(load_cfg("geballe_with_diamond_aniso"))
    c["mats"]["o_diam"][key] = block
    names = rf"mats\.g_ins\.k_aniso.*mats\.o_diam\.{key}"
    with pytest.raises(ValueError, match=names):                                 # no mesh folder, no backend: neither is reached
        run_simulation_impl("with_diamond", c, str(tmp_path / "no_mesh"), output_folder=str(tmp_path / "out"), suppress_print=True)
    with pytest.raises(ValueError, match=names):
        run_simulation_batch_impl("with_diamond", [load_cfg("geballe_with_diamond_aniso"), c],
                                  [str(tmp_path / "a"), str(tmp_path / "b")], [None, None], Untouched())
    assert not any((tmp_path / d).exists() for d in ("no_mesh", "out", "a", "b"))
    bad = copy.deepcopy(load_cfg("geballe_with_diamond"))
    bad["mats"]["p_sample"]["k_aniso"] = {"r": -1.0}
    with pytest.raises(ValueError, match=r"mats\.p_sample\.k_aniso"):
        run_simulation_impl("with_diamond", bad, str(tmp_path / "no_mesh"), suppress_print=True)


def test_used_config_carries_the_key_only_when_set():
    from heatflow_amd.driver import _with_scheme

    out = _with_scheme(load_cfg("geballe_with_diamond_aniso"))
    assert out["mats"]["p_ins"]["k_aniso"] == {"r": 2.0, "z": 0.25}
    assert "k_aniso" not in out["mats"]["p_sample"]
    plain = _with_scheme(load_cfg("geballe_with_diamond"))
    assert all("k_aniso" not in m for m in plain["mats"].values()) and "k_aniso" not in plain


class RecordingBackend:
    """Records the HeatflowHIP calls HeatProblem makes, with their arguments."""

    def __init__(self):
        self.calls, self.args = [], {}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def rec(*a, **k):
            self.calls.append(name)
            self.args[name] = a
            return None
        return rec


def _problem(small, backend, **kw):
    from helpers import make_problem

    cfg, stack, mesh = small
    return make_problem(cfg, stack, mesh, backend=backend, **kw)


def test_heat_problem_sets_the_anisotropy_after_the_materials_and_before_the_assembly(small):
    with_a, without = RecordingBackend(), RecordingBackend()
    p = _problem(small, with_a, k_aniso={3: (2.0, 0.25), np.int32(4): [1, 4]})
    _problem(small, without)
    assert without.calls == ["set_mesh", "set_materials", "set_dirichlet", "set_precond", "assemble", "set_state"]
    assert with_a.calls == ["set_mesh", "set_materials", "set_anisotropy", "set_dirichlet", "set_precond", "assemble", "set_state"]
    assert with_a.args["set_anisotropy"] == ({3: (2.0, 0.25), 4: (1.0, 4.0)},)
    assert p.k_aniso == {3: (2.0, 0.25), 4: (1.0, 4.0)}
    empty = RecordingBackend()
    _problem(small, empty, k_aniso={})
    assert empty.calls == without.calls


def test_heat_problem_refuses_bad_multipliers_and_tables_before_any_backend_call(small):
    for bad in ({3: (2.0,)}, {3: (0.0, 1.0)}, {3: (1.0, -2.0)}, {3: (np.nan, 1.0)}, {3: (np.inf, 1.0)}, {3: 2.0}):
        b = RecordingBackend()
        with pytest.raises(ValueError, match="k_aniso"):
            _problem(small, b, k_aniso=bad)
        assert b.calls == []
    for kw in ({"kappa_tables": {3: (300.0, 10.0, [1.0, 2.0])}}, {"rhoc_tables": {3: (300.0, 10.0, [1.0, 2.0])}}):
        b = RecordingBackend()
        with pytest.raises(ValueError, match=r"k_aniso.*kappa_tables.*rhoc_tables"):
            _problem(small, b, k_aniso={3: (2.0, 0.25)}, **kw)
        assert b.calls == []


# ---- drivers -----------------------------------------------------------------------------------------------------------------
def _aniso_cfg(scale=8.0):
    from heatflow_amd.geometry import scale_mesh_sizes

    return scale_mesh_sizes(load_cfg("geballe_with_diamond_aniso"), scale)


def _oracle_backend():
    """OracleBackend whose operator carries the multipliers of set_anisotropy (tests/aniso_oracle.py)."""
    import scipy.sparse.linalg as spla

    from oracle_backend import OracleBackend

    class AnisoOracleBackend(OracleBackend):
        aniso = None
        anisotropy_calls = 0

        def set_mesh(self, *a, **k):              # hf_set_mesh clears the multipliers
            self.aniso = None
            super().set_mesh(*a, **k)

        def set_anisotropy(self, multipliers):
            self.aniso = dict(multipliers)
            self.anisotropy_calls += 1

        def assemble(self, dt, mode=0):
            self._dt = dt
            self.M, self.A, self.K = operator(self.coords, self.tris, self.tags, self.tag_to_k, self.tag_to_rc, self.aniso, dt)
            self.nnz = self.A.nnz
            self.Ahat = ho.eliminate_dirichlet(self.A, self.bc_dofs) if self.n_bc else self.A
            self.A_lift = self.A[:, self.bc_dofs].tocsr() if self.n_bc else None
            self._lu = spla.splu(self.Ahat.tocsc())
            self.assemble_calls += 1

    return AnisoOracleBackend()


def test_session_carries_the_anisotropy_into_runs_and_batches(small):
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    cfg = _aniso_cfg()
    cfg["timing"]["num_steps"] = 100
    stack = build_stack(cfg)
    be = _oracle_backend()
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=be, precond=0)
    res = s.run(cfg, stack, get_watcher_points(cfg))
    assert be.anisotropy_calls == 1
    assert be.aniso == {mesh.material_tags[m]: (2.0, 0.25) for m in ("p_ins", "o_ins", "g_ins")}
    # the same run through the restatement
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 100)
    f = aniso_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, be.aniso)
    from heatflow_amd.solver import nearest_nodes

    wp = get_watcher_points(cfg)
    node = nearest_nodes(mesh.coords, [wp["oside"]] if isinstance(wp, dict) else [wp[1]])[0]
    assert np.abs(np.asarray(res["watchers"]["oside"]) - f[:, node]).max() <= 1e-9
    # a second run of the same configuration reuses the resident problem; an isotropic one builds a new problem
    s.run(cfg, stack, get_watcher_points(cfg))
    assert be.anisotropy_calls == 1 and be.set_mesh_calls == 1
    iso = copy.deepcopy(cfg)
    for m in iso["mats"].values():
        m.pop("k_aniso", None)
    res0 = s.run(iso, build_stack(iso), get_watcher_points(iso))
    assert be.set_mesh_calls == 2
    assert np.abs(np.asarray(res0["watchers"]["oside"]) - np.asarray(res["watchers"]["oside"])).max() > 1.0
    # batches: the columns must share the multipliers
    c2 = copy.deepcopy(cfg)
    c2["mats"]["p_sample"]["k"] = 4.4
    out = s.run_batch([cfg, c2], [stack, build_stack(c2)], get_watcher_points(cfg))
    assert np.abs(np.asarray(out[0]["watchers"]["oside"]) - np.asarray(res["watchers"]["oside"])).max() <= 1e-9
    with pytest.raises(ValueError, match="k_aniso"):
        s.run_batch([cfg, iso], [stack, build_stack(iso)], get_watcher_points(cfg))


def test_tangents_fit_and_1d_refuse_an_anisotropic_material(small, tmp_path):
    from heatflow_amd import fit, run_no_diamond_1d
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    cfg = _aniso_cfg()
    stack = build_stack(cfg)
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=_oracle_backend(), precond=0)
    with pytest.raises(ValueError, match=r"tangent.*mats\.p_ins\.k_aniso"):
        s.run(cfg, stack, get_watcher_points(cfg), tangents=["p_sample", "p_ins"])
    with pytest.raises(ValueError, match=r"fit.*mats\.o_ins\.k_aniso"):
        fit.fit_parameters(cfg, str(tmp_path), params=("o_ins",))
    with pytest.raises(ValueError, match=r"1-D model.*mats\.g_ins\.k_aniso"):
        run_no_diamond_1d.run_1d(cfg, str(tmp_path))


def test_header_declares_and_backend_lists_the_entry_point():
    from heatflow_amd import hip_backend
    from heatflow_amd.solver import HeatProblem

    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+hf_set_anisotropy\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int32_t\s+n\s*,\s*const\s+int32_t\s*\*\s*tags\s*,"
                     r"\s*const\s+double\s*\*\s*m_z\s*,\s*const\s+double\s*\*\s*m_r\s*\)", text)
    assert "hf_set_anisotropy" in hip_backend.EXPORTS
    assert hasattr(hip_backend.load_library(), "hf_set_anisotropy")
    assert hasattr(hip_backend.HeatflowHIP, "set_anisotropy")
    import inspect

    assert "k_aniso" in inspect.signature(HeatProblem.__init__).parameters
