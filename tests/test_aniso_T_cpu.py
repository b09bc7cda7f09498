"""Tables on anisotropic materials without a GPU (timing.aniso_tables / hf_set_aniso_tables): the restatement of
tests/aniso_T_oracle.py against the two restatements it composes (bit for bit where it degenerates to one of them), the stretch
identity under tables, two problems that separate the directions, the configuration key with everything that stays refused,
used_config.yaml, the example configuration, HeatProblem's call order and the header."""
import copy
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import aniso_oracle
import rhoc_T_oracle
from aniso_T_oracle import BDF2, BE, aniso_t_fields, operators, picard_steady, scaled_tables, stiffness
from aniso_oracle import mixed_multipliers, stretched
from conftest import ROOT, build_case, load_cfg
from kappa_T_oracle import problem_inputs
from rhoc_T_oracle import einstein_tables, rhoc_t_fields
from test_aniso_cpu import _grid

STRETCH_ENTRY_TOL = 1e-13      # of |M_ij| + dt |K_ij|
STRETCH_FIELD_TOL_K = 1e-9
NSTEPS = 20

OLD_CONFIG_TEXT = "are not supported together with temperature-dependent coefficients"
OLD_REASON = "the table kernels are isotropic"


@pytest.fixture(scope="module")
def small():
    return build_case("geballe_with_diamond", 8.0)


@pytest.fixture(scope="module")
def small_nd():
    return build_case("geballe_no_diamond", 8.0)


def _ins_tags(stack, mesh):
    return [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")]


def _ins_tables(stack, mesh, tag_to_k):
    """1/T tables for the pressure media, 300..800 K at 51 knots: the heated run crosses them (tests/test_gpu_kappa_T.py)."""
    tags = [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")]
    T = 300.0 + 10.0 * np.arange(51)
    return {t: (300.0, 10.0, tag_to_k[t] * 300.0 / T) for t in tags}


def _state(mesh, seed=3):
    """A non-uniform state inside the tables' range."""
    return 300.0 + 450.0 * np.random.default_rng(seed).random(len(mesh.coords))


# ---- 1, 2: the restatement degenerates to the restatements it composes, bit for bit --------------------------------------------
def test_unit_or_absent_multipliers_equal_the_table_restatement_bit_for_bit(small):
    cfg, stack, mesh = small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 6)
    kt, ct = _ins_tables(stack, mesh, tk), einstein_tables(trc, _ins_tags(stack, mesh))
    x = _state(mesh)
    M0, A0 = rhoc_T_oracle.operators(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, x, kt, ct)
    for aniso in (None, {}, {t: (1.0, 1.0) for t in tk}):
        M, A, _ = operators(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, x, kt, ct, aniso)
        assert np.array_equal(M.data, M0.data) and np.array_equal(A.data, A0.data)
        assert np.array_equal(M.indices, M0.indices) and np.array_equal(A.indices, A0.indices)
    for scheme, picard in ((BE, 1), (BDF2, 2)):
        f0, c0 = rhoc_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, ct, kt, scheme, picard)
        f, c = aniso_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, ct, kt, {t: (1.0, 1.0) for t in tk}, scheme, picard)
        assert np.array_equal(f, f0) and np.array_equal(c, c0)
    # the tables matter at this state: the constant-coefficient operator is another one
    _, Ac = rhoc_T_oracle.operators(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, x)
    assert np.array_equal(A0.indices, Ac.indices) and (np.abs(A0.data - Ac.data) / np.abs(Ac.data)).max() > 1e-3


def test_without_tables_the_restatement_is_the_anisotropic_one_bit_for_bit(small):
    cfg, stack, mesh = small
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, 6)
    aniso = mixed_multipliers(mesh)
    M0, A0, K0 = aniso_oracle.operator(mesh.coords, mesh.tris, mesh.tags, tk, trc, aniso, dt)
    M, A, K = operators(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, _state(mesh), None, None, aniso)
    for X, X0 in ((M, M0), (A, A0), (K, K0)):
        assert np.array_equal(X.data, X0.data) and np.array_equal(X.indices, X0.indices)
    for scheme in (BE, BDF2):
        f0 = aniso_oracle.aniso_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, aniso, scheme)
        f, _ = aniso_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, None, None, aniso, scheme, 1)
        # (the loops differ in one place only: aniso_fields factorises once, this one per step - the same matrix, the same bits)
        assert np.array_equal(f, f0)


# ---- 3: stretch identity under tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("picard", [1, 3])
@pytest.mark.parametrize("which", ["small", "small_nd"])
def test_stretch_identity_under_tables(request, which, picard):
    """Every tag at m_r = 1, m_z = 1/4 with tables = the isotropic problem on (2 z, r) with k / 2, rho_c / 2 and every table value
    halved: the substitution of aniso_oracle.stretched holds element by element, whatever kappa_e and rho_c_e are, and T_e does
    not see the coordinates."""
    cfg, stack, mesh = request.getfixturevalue(which)
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, NSTEPS)
    kt, ct = _ins_tables(stack, mesh, tk), einstein_tables(trc, _ins_tags(stack, mesh))
    s = 2.0
    aniso = {t: (1.0, 1.0 / (s * s)) for t in tk}
    cs, ks, rcs = stretched(mesh.coords, tk, trc, s)
    kts, cts = scaled_tables(kt, s), scaled_tables(ct, s)
    x = _state(mesh)
    M, A, K = operators(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, x, kt, ct, aniso)
    Ms, As, Ks = operators(cs, mesh.tris, mesh.tags, ks, rcs, dt, x, kts, cts, None)
    scale = abs(M) + dt * abs(K)
    for X, Xs in ((M, Ms), (A, As), (dt * K, dt * Ks)):
        D = abs(X - Xs).tocsr()
        worst = (D.data / np.asarray(scale[D.nonzero()]).ravel()).max() if D.nnz else 0.0
        print(f"{which}: worst entry difference / (|M| + dt |K|) = {worst:.2e}")
        assert worst <= STRETCH_ENTRY_TOL
    f, _ = aniso_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, ct, kt, aniso, BE, picard)
    fs, _ = rhoc_t_fields(cs, mesh.tris, mesh.tags, ks, rcs, dt, dofs, u0, g, cts, kts, BE, picard)
    iso, _ = rhoc_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, ct, kt, BE, picard)
    worst, moved = float(np.abs(f - fs).max()), float(np.abs(f - iso).max())
    print(f"{which} picard={picard}: fields differ by {worst:.2e} K; the anisotropy moves the field under tables by {moved:.1f} K")
    assert worst <= STRETCH_FIELD_TOL_K
    assert moved > 1.0


# ---- 4: directions ---------------------------------------------------------------------------------------------------------------
def test_stiffness_at_a_field_of_r_alone_ignores_m_z_under_tables():
    """The two-shell mesh of tests/test_aniso_cpu.py: a nodal field that depends on r alone has no z-gradient on any triangle, and
    kappa_e(T_e) does not see the multipliers, so K(m_z)(u) u = K(m_z')(u) u to rounding - with 1/T tables on both shells."""
    a, c, b = 1e-6, 2e-6, 4e-6
    r = np.concatenate([np.linspace(a, c, 33), np.linspace(c, b, 65)[1:]])
    z = np.linspace(0.0, 1e-6, 5)
    coords, tris, tags = _grid(z, r, lambda zc, rc: 1 if rc < c else 2)
    tk = {1: 10.0, 2: 3.0}
    T = 300.0 + 10.0 * np.arange(51)
    kt = {t: (300.0, 10.0, tk[t] * 300.0 / T) for t in tk}
    rng = np.random.default_rng(5)
    u_r = (300.0 + 400.0 * rng.random(len(r)))[np.searchsorted(r, coords[:, 1])]
    Ks = {mz: stiffness(coords, tris, tags, tk, u_r, kt, {1: (2.0, mz), 2: (0.5, 1.0 / mz)}) for mz in (1.0, 1.0 / 16.0, 16.0)}
    for mz in (1.0 / 16.0, 16.0):
        err = np.abs(Ks[mz] @ u_r - Ks[1.0] @ u_r)
        bound = 1e-13 * (abs(Ks[1.0]) @ np.abs(u_r))
        print(f"m_z = {mz}: worst |K u - K_1 u| / (|K| |u|) = {(err / (bound / 1e-13)).max():.2e}")
        assert np.all(err <= bound)
        assert abs(Ks[mz] - Ks[1.0]).max() > 1e-3 * abs(Ks[1.0]).max()            # (the matrices themselves differ)
    # ... and the tables are felt: the constant-coefficient stiffness gives another product
    K_const = stiffness(coords, tris, tags, tk, u_r, None, {1: (2.0, 1.0), 2: (0.5, 1.0)})
    assert np.abs(K_const @ u_r - Ks[1.0] @ u_r).max() > 1e-3 * np.abs(Ks[1.0] @ u_r).max()


def test_picard_steady_state_of_a_layered_slab_ignores_m_r_under_a_table():
    """Two layers stacked along z between held faces, the first with a 1/T table; m_r = 1 against m_r = 7.
    What is exact, and asserted: a Picard sweep from a state that is uniform per layer values kappa uniformly per layer, its
    solution is the piecewise linear profile - a member of the P1 space - and the radial conductivity never enters: the sweep's
    answer does not move with m_r (1e-9 K), while the table (kappa at 500 K, not the constant) and m_z do move it.  And at any
    state that depends on z alone the product K(x) x does not depend on m_r (1e-13 of |K| |x|), whatever the table makes of
    kappa_e: that state has no r-gradient on any triangle.
    What is not exact, and only printed: the converged fixed point.  From the second sweep on the two triangle orientations of a
    column of the grid have different T_e, (2 x_i + x_{i+1}) / 3 and (x_i + 2 x_{i+1}) / 3, hence different kappa_e; the rows of
    the first and the last node row of the grid see one orientation each, the rows between them both, so no P1 field of z alone
    solves the sweep's system, the iterate picks up an r-gradient of the order of the z-step's share of the table's slope, and
    with it a dependence on m_r.  Measured on this 8 x 6 grid, 700 K to 300 K: 0.13 K (m_z = 1) and 0.18 K (m_z = 1/4)
    between m_r = 1 and 7, and 0.16 K with the grid moved 1 m to 10 km away from the axis (so it is not the r-weight), against
    57 K that the table moves the field.  That is a property of
    P1 elements with one kappa per element, of the isotropic table path as much as of this one (there it shows as an r-dependence
    of a slab's field), not of the multipliers."""
    z = np.linspace(0.0, 4e-6, 9)
    r = np.linspace(0.0, 3e-6, 7)
    coords, tris, tags = _grid(z, r, lambda zc, rc: 1 if zc < 2e-6 else 2)
    tk = {1: 10.0, 2: 3.0}
    T = 300.0 + 10.0 * np.arange(51)
    kt = {1: (300.0, 10.0, tk[1] * 300.0 / T)}
    lo, hi = np.nonzero(coords[:, 0] == z[0])[0], np.nonzero(coords[:, 0] == z[-1])[0]
    mid = np.nonzero(coords[:, 0] == 2e-6)[0]
    dofs = np.concatenate([lo, hi])
    g = np.concatenate([np.full(len(lo), 700.0), np.full(len(hi), 300.0)])
    x0 = np.full(len(coords), 500.0)
    one, full = {}, {}
    for m_r in (1.0, 7.0):
        for m_z in (1.0, 0.25):
            an = {1: (m_r, m_z), 2: (1.0 / m_r, 1.0)}
            one[(m_r, m_z)] = picard_steady(coords, tris, tags, tk, dofs, g, x0, kt, an, max_sweeps=1)["u"]
            full[(m_r, m_z)] = picard_steady(coords, tris, tags, tk, dofs, g, x0, kt, an, picard_tol=1e-11, max_sweeps=100)
            assert full[(m_r, m_z)]["converged"]
    for m_z in (1.0, 0.25):
        d = float(np.abs(one[(1.0, m_z)] - one[(7.0, m_z)]).max())
        R1, R2 = 2e-6 / (m_z * tk[1] * 300.0 / 500.0), 2e-6 / tk[2]               # the series resistances at kappa_1(500 K)
        t_int = 700.0 - 400.0 * R1 / (R1 + R2)
        print(f"m_z = {m_z}: one sweep, m_r = 1 against m_r = 7: {d:.2e} K; interface {one[(1.0, m_z)][mid].mean():.6f} K "
              f"(series resistance {t_int:.6f} K)")
        assert d <= 1e-9
        assert np.abs(one[(1.0, m_z)][mid] - t_int).max() <= 1e-9                   # the table's kappa(500 K), m_z times it
        dfull = float(np.abs(full[(1.0, m_z)]["u"] - full[(7.0, m_z)]["u"]).max())
        print(f"m_z = {m_z}: the fixed points differ by {dfull:.2e} K ({full[(1.0, m_z)]['sweeps']} and {full[(7.0, m_z)]['sweeps']} "
              f"sweeps): the discretisation's r-dependence, see the docstring")
    assert np.abs(one[(1.0, 1.0)] - one[(1.0, 0.25)]).max() > 10.0                  # m_z does move it
    # the r-dependence is the discretisation's, not the multipliers': the isotropic table path's fixed point (no multipliers at
    # all) varies along r too, far above the 1e-9 K of the solves, while its first sweep from the uniform state does not
    iso = picard_steady(coords, tris, tags, tk, dofs, g, x0, kt, None, picard_tol=1e-11, max_sweeps=100)
    iso1 = picard_steady(coords, tris, tags, tk, dofs, g, x0, kt, None, max_sweeps=1)["u"]
    spread = lambda u: float(np.ptp(u.reshape(len(z), len(r)), axis=1).max())       # largest variation along r over the columns
    print(f"isotropic table path: the fixed point varies along r by {spread(iso['u']):.2e} K, its first sweep by {spread(iso1):.2e} K; "
          f"anisotropic (m_r = 1, m_z = 1/4): {spread(full[(1.0, 0.25)]['u']):.2e} K")
    assert iso["converged"] and spread(iso["u"]) > 1e-6 and spread(iso1) <= 1e-9
    const = picard_steady(coords, tris, tags, tk, dofs, g, x0, None, {1: (1.0, 0.25), 2: (1.0, 1.0)}, max_sweeps=1)["u"]
    assert np.abs(const - one[(1.0, 0.25)]).max() > 10.0                            # and so does the table
    # K(x) x at a state of z alone, the table evaluated element by element
    rng = np.random.default_rng(9)
    x_z = (300.0 + 400.0 * rng.random(len(z)))[np.searchsorted(z, coords[:, 0])]
    Ks = {m_r: stiffness(coords, tris, tags, tk, x_z, kt, {1: (m_r, 0.25), 2: (1.0 / m_r, 1.0)}) for m_r in (1.0, 7.0)}
    err = np.abs(Ks[7.0] @ x_z - Ks[1.0] @ x_z)
    scale = abs(Ks[1.0]) @ np.abs(x_z)
    print(f"worst |K(m_r = 7) x - K(m_r = 1) x| / (|K| |x|) at a state of z alone = {(err / scale).max():.2e}")
    assert np.all(err <= 1e-13 * scale)
    assert abs(Ks[7.0] - Ks[1.0]).max() > 1e-3 * abs(Ks[1.0]).max()                 # (the matrices themselves differ)


# ---- 5: configuration ----------------------------------------------------------------------------------------------------------
def _both_cfg(scale=8.0):
    from heatflow_amd.geometry import scale_mesh_sizes

    return scale_mesh_sizes(load_cfg("geballe_with_diamond_aniso_kT"), scale)


TABLE_BLOCKS = [("k_table", {"T_min": 300.0, "T_max": 700.0, "k": [4.0, 3.0]}),
                ("k_power", {"T_ref": 300.0, "exponent": 1.0, "T_min": 300.0, "T_max": 900.0}),
                ("cv_table", {"T_min": 300.0, "T_max": 700.0, "cv": [600.0, 700.0]}),
                ("cv_einstein", {"theta": 600.0, "T_ref": 300.0, "T_min": 300.0, "T_max": 900.0})]


def test_the_key_parses_and_a_non_boolean_is_refused_naming_it():
    from heatflow_amd.aniso import aniso_tables, check_config

    assert aniso_tables({}) is False and aniso_tables({"timing": {}}) is False and aniso_tables({"timing": None}) is False
    assert aniso_tables({"timing": {"aniso_tables": True}}) is True
    assert aniso_tables({"timing": {"aniso_tables": False}}) is False
    assert aniso_tables(load_cfg("geballe_with_diamond_aniso_kT")) is True
    for other in ("geballe_with_diamond", "geballe_with_diamond_aniso", "geballe_with_diamond_kT"):
        assert aniso_tables(load_cfg(other)) is False
    for bad in (1, 0, "true", "yes", None, [True]):
        c = copy.deepcopy(load_cfg("geballe_with_diamond"))
        c["timing"]["aniso_tables"] = bad
        with pytest.raises(ValueError, match=r"timing\.aniso_tables must be true or false"):
            aniso_tables(c)
        with pytest.raises(ValueError, match=r"timing\.aniso_tables"):
            check_config(c)


@pytest.mark.parametrize("where", ["same", "other"])
@pytest.mark.parametrize("key,block", TABLE_BLOCKS)
def test_check_config_refuses_as_before_without_the_key_and_accepts_with_it(key, block, where):
    from heatflow_amd.aniso import check_config
    from heatflow_amd.geometry import build_stack

    c = copy.deepcopy(load_cfg("geballe_with_diamond_aniso"))
    mat = "g_ins" if where == "same" else "o_diam"
    c["mats"][mat][key] = block
    for off in ({}, {"aniso_tables": False}):
        c0 = copy.deepcopy(c)
        c0["timing"].update(off)
        with pytest.raises(ValueError, match=rf"mats\.g_ins\.k_aniso.*{OLD_CONFIG_TEXT}.*mats\.{mat}\.{key}.*{OLD_REASON}"):
            check_config(c0)
        with pytest.raises(ValueError, match=OLD_CONFIG_TEXT):
            build_stack(c0)
    c["timing"]["aniso_tables"] = True
    assert check_config(c) == {m: (2.0, 0.25) for m in ("g_ins", "o_ins", "p_ins")}
    stack = build_stack(c)
    assert stack.by_name("g_ins").properties["k_aniso"] == (2.0, 0.25)
    prop = {"k_table": "k_table", "k_power": "k_table", "cv_table": "rho_cv_table", "cv_einstein": "rho_cv_table"}[key]
    assert prop in stack.by_name(mat).properties


def test_the_drivers_refuse_as_before_without_the_key(tmp_path):
    from heatflow_amd.driver import run_simulation_batch_impl, run_simulation_impl

    class Untouched:                                                             # any use of the session is an AttributeError
        pass

    c = load_cfg("geballe_with_diamond_aniso_kT")
    del c["timing"]["aniso_tables"]
    names = rf"mats\.g_ins\.k_aniso.*{OLD_CONFIG_TEXT}.*mats\.g_ins\.k_power.*{OLD_REASON}"
    for kind in ("with_diamond", "no_diamond"):
        with pytest.raises(ValueError, match=names):                             # no mesh folder, no backend: neither is reached
            run_simulation_impl(kind, c, str(tmp_path / "no_mesh"), output_folder=str(tmp_path / "out"), suppress_print=True)
        with pytest.raises(ValueError, match=names):
            run_simulation_batch_impl(kind, [c, c], [str(tmp_path / "a"), str(tmp_path / "b")], [None, None], Untouched())
    assert not any((tmp_path / d).exists() for d in ("no_mesh", "out", "a", "b"))


class RecordingBackend:
    """Records the HeatflowHIP calls HeatProblem makes, with their arguments (the style of tests/oracle_backend.py's stand-in)."""

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


def test_heat_problem_refuses_as_before_and_orders_the_calls_under_the_switch(small):
    an = {3: (2.0, 0.25)}
    kt, ct = {3: (300.0, 10.0, [1.0, 2.0])}, {4: (300.0, 10.0, [1.0, 2.0])}
    for kw in ({"kappa_tables": kt}, {"rhoc_tables": ct}, {"kappa_tables": kt, "aniso_tables": False}):
        b = RecordingBackend()
        with pytest.raises(ValueError, match=rf"HeatProblem: k_aniso together with kappa_tables / rhoc_tables is not supported \({OLD_REASON}\)"):
            _problem(small, b, k_aniso=an, **kw)
        assert b.calls == []
    b = RecordingBackend()
    p = _problem(small, b, k_aniso=an, kappa_tables=kt, rhoc_tables=ct, picard=2, aniso_tables=True)
    assert b.calls == ["set_mesh", "set_materials", "set_aniso_tables", "set_anisotropy", "set_dirichlet", "set_precond",
                       "set_kappa_tables", "set_rhoc_tables", "set_picard", "set_state", "assemble"]
    assert b.args["set_aniso_tables"] == (True,) and b.args["set_anisotropy"] == (an,) and p.aniso_tables is True
    # off (the default) makes no extra call, whatever else is set
    for kw in ({}, {"k_aniso": an}, {"kappa_tables": kt}):
        b = RecordingBackend()
        _problem(small, b, **kw)
        assert "set_aniso_tables" not in b.calls
    assert inspect.signature(type(p).__init__).parameters["aniso_tables"].default is False


def _table_oracle_backend():
    """OracleBackend that carries the switch, the multipliers and the tables into a lagged backward-Euler step (tests/aniso_T_oracle.py)."""
    import scipy.sparse.linalg as spla

    from oracle import heat_oracle as ho
    from oracle_backend import OracleBackend

    class TableOracleBackend(OracleBackend):
        def set_mesh(self, *a, **k):
            self.switch, self.aniso, self.kt, self.ct, self.order = False, None, None, None, []
            super().set_mesh(*a, **k)

        def set_aniso_tables(self, on):
            self.switch = bool(on)
            self.order.append("set_aniso_tables")

        def set_anisotropy(self, multipliers):
            assert self.switch or not (self.kt or self.ct)
            self.aniso = dict(multipliers)
            self.order.append("set_anisotropy")

        def set_kappa_tables(self, tables, picard=1):
            assert self.switch or not self.aniso
            assert picard == 1
            self.kt = dict(tables)
            self.order.append("set_kappa_tables")

        def assemble(self, dt, mode=0):
            self._dt = dt
            self.assemble_calls += 1

        def step(self, g, rtol=1e-10, atol=0.0, max_it=20000):
            M, A, _ = operators(self.coords, self.tris, self.tags, self.tag_to_k, self.tag_to_rc, self._dt, self.u, self.kt, self.ct,
                                self.aniso)
            b = M @ self.u
            b -= A[:, self.bc_dofs].tocsr() @ g
            b[self.bc_dofs] = g
            self.u = spla.splu(ho.eliminate_dirichlet(A, self.bc_dofs).tocsc()).solve(b)
            return 1, 0.0

    return TableOracleBackend()


def test_session_carries_the_switch_into_the_problem_and_keys_the_resident_problem_by_it(small):
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points
    from heatflow_amd.solver import nearest_nodes

    _, _, mesh = small
    cfg = _both_cfg()
    nsteps = 30
    cfg["timing"]["num_steps"] = nsteps
    cfg["timing"]["t_final"] = cfg["timing"]["t_final"] * nsteps / 100
    stack = build_stack(cfg)
    be = _table_oracle_backend()
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=be, precond=0)
    wp = get_watcher_points(cfg)
    res = s.run(cfg, stack, wp)
    assert be.order == ["set_aniso_tables", "set_anisotropy", "set_kappa_tables"] and be.switch
    assert s.problem.aniso_tables is True
    assert be.aniso == {mesh.material_tags[m]: (2.0, 0.25) for m in ("p_ins", "o_ins", "g_ins")}
    assert set(be.kt) == {mesh.material_tags[m] for m in ("p_ins", "o_ins", "g_ins", "p_diam", "o_diam")}
    # the same run through the restatement
    tk, trc, dt, dofs, u0, g = problem_inputs(cfg, stack, mesh, nsteps)
    f, _ = aniso_t_fields(mesh.coords, mesh.tris, mesh.tags, tk, trc, dt, dofs, u0, g, None, be.kt, be.aniso)
    node = nearest_nodes(mesh.coords, [wp["oside"]] if isinstance(wp, dict) else [wp[1]])[0]
    assert np.abs(np.asarray(res["watchers"]["oside"]) - f[:, node]).max() <= 1e-9
    # a second run of the same configuration reuses the resident problem
    s.run(cfg, stack, wp)
    assert be.set_mesh_calls == 1
    # the key carries the switch: the same problem without it is another resident problem
    from heatflow_amd.driver import ProblemSpec

    base = ProblemSpec(1.0, "backward_euler", {1: 2.0}, [], k_aniso={1: (2.0, 0.25)})
    assert dataclasses.replace(base, aniso_tables=False).key == base.key
    assert dataclasses.replace(base, aniso_tables=True).key != base.key
    assert "aniso_tables" not in base.problem_kwargs()
    assert dataclasses.replace(base, aniso_tables=True).problem_kwargs()["aniso_tables"] is True
    only_an = copy.deepcopy(cfg)
    for m in only_an["mats"].values():
        m.pop("k_power", None)
    s.run(only_an, build_stack(only_an), wp)                                      # (the switch stays set: still accepted)
    assert be.set_mesh_calls == 2 and be.kt is None and be.switch
    del only_an["timing"]["aniso_tables"]
    s.run(only_an, build_stack(only_an), wp)
    assert be.set_mesh_calls == 3 and not be.switch and be.order == ["set_anisotropy"]


def test_refusals_that_stay_under_the_key_name_their_key(small, tmp_path):
    import yaml

    from heatflow_amd import fit, parameter_sweep, run_no_diamond_1d
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    cfg = _both_cfg()
    stack = build_stack(cfg)
    be = _table_oracle_backend()
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=be, precond=0)
    wp = get_watcher_points(cfg)
    both = r"timing\.aniso_tables.*mats\.g_ins\.k_aniso.*mats\.g_ins\.k_power"
    for extra in ({}, {"table_tangents": True}):                                  # with timing.table_tangents too
        c = copy.deepcopy(cfg)
        c["timing"].update(extra)
        with pytest.raises(ValueError, match="tangents: " + both):
            s.run(c, stack, wp, tangents=["p_sample"])
        with pytest.raises(ValueError, match="tangents: " + both):
            s.run(c, stack, wp, tangents=["p_ins.k_r"])
        cm = copy.deepcopy(c)
        cm["monitors"] = {"sample": {"material": "p_sample"}}
        with pytest.raises(ValueError, match="monitor_sigma: " + both):
            s.run(cm, stack, wp, monitor_sigma={"p_sample": 0.1})
        with pytest.raises(ValueError, match=r"heatflow_amd\.fit: " + both):
            fit.fit_parameters(c, str(tmp_path), params=("p_sample",))
    assert be.set_mesh_calls == 0                                                 # all before any problem was made
    # the sweeps and run_batch refuse tables anyway and keep their messages
    with pytest.raises(ValueError, match=r"run_batch \(the batched loop\) does not support temperature-dependent conductivities \(mats\.g_ins\.k_power"):
        s.run_batch([cfg, cfg], [stack, stack], wp)
    with pytest.raises(ValueError, match=r"run_kappa_sweep does not support temperature-dependent conductivities \(mats\.g_ins\.k_power"):
        parameter_sweep.run_kappa_sweep(cfg, str(tmp_path), [3.8], str(tmp_path))
    p = tmp_path / "c.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with pytest.raises(ValueError, match=r"run_parameter_sweep does not support temperature-dependent conductivities \(mats\.g_ins\.k_power"):
        parameter_sweep.run_parameter_sweep(str(p), str(tmp_path), [1e-5, 1e-5], [3.8, 3.8], [1.84e-6, 1.84e-6], 1)
    # the 1-D model: the table key first, as before, and the anisotropy key once the tables are gone
    with pytest.raises(ValueError, match=r"1-D model.*mats\.g_ins\.k_power"):
        run_no_diamond_1d.run_1d(cfg, str(tmp_path))
    c = copy.deepcopy(cfg)
    for m in c["mats"].values():
        m.pop("k_power", None)
    with pytest.raises(ValueError, match=r"1-D model.*mats\.g_ins\.k_aniso"):
        run_no_diamond_1d.run_1d(c, str(tmp_path))
    # a non-boolean value
    c = copy.deepcopy(cfg)
    c["timing"]["aniso_tables"] = "yes"
    with pytest.raises(ValueError, match=r"timing\.aniso_tables must be true or false"):
        s.run(c, stack, wp)
    with pytest.raises(ValueError, match=r"timing\.aniso_tables must be true or false"):
        build_stack(c)


def test_fit_and_tangents_refuse_as_before_without_the_key(small, tmp_path):
    """Without timing.aniso_tables the new refusal is silent: a configuration with both kinds meets the messages of before."""
    from heatflow_amd import fit
    from heatflow_amd.aniso import refuse_aniso_tables
    from heatflow_amd.driver import SimulationSession
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small
    keyed = _both_cfg()
    stack = build_stack(keyed)                                                    # (the stack itself needs the key)
    wp = get_watcher_points(keyed)
    be = _table_oracle_backend()
    s = SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=be, precond=0)
    for off in (None, False):
        cfg = copy.deepcopy(keyed)
        if off is None:
            del cfg["timing"]["aniso_tables"]
        else:
            cfg["timing"]["aniso_tables"] = False
        refuse_aniso_tables(cfg, "anything")                                      # raises nothing
        old = r"does not support temperature-dependent conductivities \(mats\.g_ins\.k_power, mats\.o_diam\.k_power"
        with pytest.raises(ValueError, match="^heatflow_amd.fit " + old) as e:
            fit.fit_parameters(cfg, str(tmp_path), params=("p_sample",))
        assert "aniso_tables" not in str(e.value)
        with pytest.raises(ValueError, match="^tangents " + old) as e:
            s.run(cfg, stack, wp, tangents=["p_sample"])
        assert "aniso_tables" not in str(e.value)
        cm = copy.deepcopy(cfg)
        cm["monitors"] = {"sample": {"material": "p_sample"}}
        with pytest.raises(ValueError, match="^tangents " + old) as e:
            s.run(cm, stack, wp, monitor_sigma={"p_sample": 0.1})
        assert "aniso_tables" not in str(e.value)
    assert be.set_mesh_calls == 0


def test_used_config_round_trips_and_writes_the_key_only_when_set(tmp_path):
    import yaml

    from heatflow_amd.aniso import aniso_tables, check_config
    from heatflow_amd.driver import _dump_yaml, _with_scheme

    out = _with_scheme(load_cfg("geballe_with_diamond_aniso_kT"))
    assert out["timing"]["aniso_tables"] is True
    assert out["mats"]["p_ins"]["k_aniso"] == {"r": 2.0, "z": 0.25} and "k_power" in out["mats"]["p_ins"]
    assert set(out["kappa_tables"]) == {"p_ins", "o_ins", "g_ins", "p_diam", "o_diam"}
    path = tmp_path / "used_config.yaml"
    with open(path, "w") as f:
        _dump_yaml(out, f)
    with open(path) as f:
        back = yaml.safe_load(f)
    assert aniso_tables(back) is True
    assert check_config(back) == check_config(load_cfg("geballe_with_diamond_aniso_kT"))
    assert _with_scheme(back)["timing"] == out["timing"] and _with_scheme(back)["kappa_tables"] == out["kappa_tables"]
    for other in ("geballe_with_diamond", "geballe_with_diamond_aniso", "geballe_with_diamond_kT", "geballe_with_diamond_cvT"):
        assert "aniso_tables" not in _with_scheme(load_cfg(other))["timing"]


def test_the_example_configuration_loads_and_is_the_two_parent_examples_together():
    from heatflow_amd.geometry import build_stack

    cfg = load_cfg("geballe_with_diamond_aniso_kT")
    an, kt = load_cfg("geballe_with_diamond_aniso"), load_cfg("geballe_with_diamond_kT")
    with open(os.path.join(ROOT, "cfgs", "geballe_with_diamond_aniso_kT.yaml")) as f:
        assert "ILLUSTRATIVE" in f.readline()
    stack = build_stack(cfg)
    for name, mat in cfg["mats"].items():
        assert mat.get("k_aniso") == an["mats"][name].get("k_aniso")
        assert mat.get("k_power") == kt["mats"][name].get("k_power")
        assert {k: v for k, v in mat.items() if k not in ("k_aniso", "k_power")} == \
            {k: v for k, v in an["mats"][name].items() if k != "k_aniso"}
    for name in ("g_ins", "o_ins", "p_ins"):                                     # both kinds on the same materials
        props = stack.by_name(name).properties
        assert props["k_aniso"] == (2.0, 0.25) and "k_table" in props
    assert cfg["timing"] == dict(kt["timing"], aniso_tables=True) and cfg["heating"] == an["heating"]


def test_header_declares_and_backend_lists_the_entry_point():
    from heatflow_amd import hip_backend
    from heatflow_amd.solver import HeatProblem

    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+hf_set_aniso_tables\s*\(\s*hf_ctx\s*\*\s*ctx\s*,\s*int32_t\s+on\s*\)", text)
    assert "hf_set_aniso_tables" in hip_backend.EXPORTS
    assert hasattr(hip_backend.load_library(), "hf_set_aniso_tables")
    assert hasattr(hip_backend.HeatflowHIP, "set_aniso_tables")
    assert "aniso_tables" in inspect.signature(HeatProblem.__init__).parameters
