"""Tangent runs and the fit built on them, without a GPU: gaussian_dfwhm against differences of gaussian, the shared sweep
objective against its former formula, and HeatProblem.run_tangent / Session.run(tangents=...) / fit_parameters driving a
scipy-backed backend that restates the tangent recursion with sparse LU solves (TangentOracleBackend, also the exact
reference of tests/test_gpu_tangent.py)."""
import copy

import numpy as np
import pytest

from conftest import HEATING_CSV, build_case
from oracle import heat_oracle as ho
from oracle_backend import OracleBackend
from test_cabi import _declared_symbols


class TangentOracleBackend(OracleBackend):
    """OracleBackend plus hf_tangent_setup / hf_run_tangent / hf_get_tangent: after each primal step, per column
    A_hat s^{n+1} = M s^n + dt F - A[:,B] h on the free rows, s_B = h, F = -K_j u^{n+1} (K_j = the unit-conductivity
    stiffness of the column's tags, un-eliminated)."""

    tangent_nv = 0

    def tangent_setup(self, n_par, tag_col):
        if not 1 <= n_par <= 16:
            raise ValueError("n_par outside 1..16")
        self.tangent_nv = next(v for v in (2, 4, 8, 16) if v >= n_par)
        col = np.full(self.tags.max() + 1, -1)
        for t, j in tag_col.items():
            col[t] = j
        self._col = col
        self._Kj = []
        for j in range(self.tangent_nv):
            ind = (col[self.tags] == j).astype(np.float64)
            self._Kj.append(ho.assemble_csr(self.n, self.tris, ho.element_matrices(self.coords, self.tris, ind, ind)[1]))
        self.S = np.zeros((self.n, self.tangent_nv))

    def _reset_tangents(self):
        if self.tangent_nv:
            self.S[:] = 0.0

    def set_state(self, u):
        super().set_state(u)
        self._reset_tangents()

    def set_materials(self, tags, kappa, rho_c):
        super().set_materials(tags, kappa, rho_c)
        self._reset_tangents()

    def assemble(self, dt, mode=0):
        super().assemble(dt, mode)
        self._reset_tangents()

    def run_tangent(self, g_all, h_all=None, rtol=1e-10, atol=0.0, max_it=20000, nodes=None):
        nv, ns = self.tangent_nv, 0 if nodes is None else len(nodes)
        nodes = None if nodes is None else np.asarray(nodes)
        nsteps = len(g_all)
        samples, tsamples = np.empty((nsteps, ns)), np.empty((nsteps, nv, ns))
        for k, g in enumerate(g_all):
            self.step(g)
            for j in range(nv):
                h = h_all[k, :, j] if h_all is not None else np.zeros(self.n_bc)
                b = self.M @ self.S[:, j] - self._dt * (self._Kj[j] @ self.u)
                if self.n_bc:
                    b -= self.A_lift @ h
                    b[self.bc_dofs] = h
                self.S[:, j] = self._lu.solve(b)
            if ns:
                samples[k] = self.u[nodes]
                tsamples[k] = self.S[nodes].T
        return samples, np.ones(nsteps, dtype=np.int32), tsamples, np.ones((nsteps, nv), dtype=np.int32)

    def get_tangent(self, j):
        return self.S[:, j].copy()


@pytest.fixture(scope="module")
def small():
    cfg, stack, mesh = build_case("geballe_with_diamond", 8.0)
    cfg = copy.deepcopy(cfg)
    cfg["timing"]["num_steps"] = 30          # same t_final, coarser steps: the fits below run a few dozen simulations
    return cfg, stack, mesh


def _session(mesh):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=TangentOracleBackend())


def _synthetic_exp(cfg, mesh, params, values):
    """Experiment columns that a run at `values` reproduces exactly: time, temp = p-side, oside = o-side."""
    from heatflow_amd.fit import set_params
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    s = _session(mesh)
    try:
        c = set_params(cfg, params, values)
        res = s.run(c, build_stack(c), get_watcher_points(c))
    finally:
        s.close()
    return {"time": res["times"], "temp": res["watchers"]["pside"], "oside": res["watchers"]["oside"]}


def test_header_declares_and_backend_lists_tangent_entry_points():
    from heatflow_amd import hip_backend

    declared = _declared_symbols()
    for name in ("hf_tangent_setup", "hf_run_tangent", "hf_get_tangent"):
        assert name in declared and name in hip_backend.EXPORTS


def test_gaussian_dfwhm_matches_central_difference():
    from heatflow_amd.heating import HeatingCurve

    r = np.linspace(0.0, 3e-5, 41)
    z = np.zeros_like(r)
    for fwhm in (1.32e-5, 8e-6):
        for t in (2.5e-6, 4e-6, 6e-6):
            hc = HeatingCurve(HEATING_CSV, 300.0, fwhm)
            d = hc.gaussian_dfwhm(z, r, t)
            eps = fwhm * 1e-5
            up, dn = HeatingCurve(HEATING_CSV, 300.0, fwhm + eps), HeatingCurve(HEATING_CSV, 300.0, fwhm - eps)
            fd = (up.gaussian(z, r, t) - dn.gaussian(z, r, t)) / (2 * eps)
            assert np.max(np.abs(d)) > 0
            np.testing.assert_allclose(d, fd, rtol=1e-7, atol=1e-7 * np.max(np.abs(fd)))


def test_shared_objective_equals_the_sweeps_former_formula():
    from heatflow_amd.analysis_utils import calculate_rmse
    from heatflow_amd.parameter_sweep import oside_rmse

    rng = np.random.default_rng(3)
    exp = np.genfromtxt(HEATING_CSV, delimiter=",", names=True)
    times = np.linspace(0.0, 7.5e-6, 100)
    ps = 300 + 900 * np.sin(np.linspace(0, 3, 100)) ** 2 + rng.normal(0, 1, 100)
    os_ = 300 + 200 * np.linspace(0, 1, 100) ** 2 + rng.normal(0, 1, 100)
    ic = 300.0
    # restatement of run_kappa_sweep's closure as it stood
    sim_o = (os_ - os_[0]) / (ps.max() - ps.min())
    exp_o = exp["oside"] - exp["oside"][0] + ic
    exp_o = (exp_o - exp_o[0]) / (exp["temp"].max() - exp["temp"].min())
    want = calculate_rmse(exp["time"], exp_o, times, sim_o)
    assert oside_rmse(exp, ic, times, ps, os_) == want


def test_run_tangent_matches_finite_differences_of_runs(small):
    """HeatProblem.run_tangent's host logic (column map, h tabulation, padding) with the restated recursion."""
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    cfg, stack, mesh = small
    s = _session(mesh)
    try:
        res = s.run(cfg, stack, get_watcher_points(cfg), tangents=("p_sample", "fwhm", "p_coupler"))
        assert set(res["tangents"]) == {"p_sample", "fwhm", "p_coupler"}
        assert res["tangent_iters"].shape == (30, 3)
        for name, rel in (("p_sample", 1e-4), ("fwhm", 1e-4)):
            base = float(cfg["heating"]["fwhm"]) if name == "fwhm" else float(cfg["mats"][name]["k"])
            curves = []
            for sgn in (1, -1):
                c = copy.deepcopy(cfg)
                v = base * (1 + sgn * 1e-4)
                if name == "fwhm":
                    c["heating"]["fwhm"] = v
                else:
                    c["mats"][name]["k"] = v
                curves.append(s.run(c, build_stack(c), get_watcher_points(c))["watchers"]["oside"])
            fd = (curves[0] - curves[1]) / (2e-4 * base)
            tan = res["tangents"][name]["oside"]
            assert np.max(np.abs(tan)) > 0
            assert np.max(np.abs(tan - fd)) <= rel * np.max(np.abs(tan))
    finally:
        s.close()


def test_fit_jacobian_matches_central_differences_of_the_residual(small):
    from heatflow_amd.fit import residual_and_jacobian, set_params
    from heatflow_amd.parameter_sweep import build_stack, get_watcher_points

    cfg, stack, mesh = small
    params = ("p_sample", "fwhm")
    exp = _synthetic_exp(cfg, mesh, params, [4.07, 1.2e-5])
    ic = float(cfg["heating"]["ic_temp"])
    theta = np.array([3.9, 1.3e-5])
    s = _session(mesh)
    try:
        c = set_params(cfg, params, theta)
        _, J = residual_and_jacobian(s.run(c, build_stack(c), get_watcher_points(c), tangents=params), params, exp, ic)
        for j in range(2):
            rs = []
            for sgn in (1, -1):
                th = theta.copy()
                th[j] *= 1 + sgn * 1e-5
                c = set_params(cfg, params, th)
                rs.append(residual_and_jacobian(s.run(c, build_stack(c), get_watcher_points(c), tangents=params), params, exp, ic)[0])
            fd = (rs[0] - rs[1]) / (2e-5 * theta[j])
            assert np.max(np.abs(J[:, j] - fd)) <= 1e-5 * np.max(np.abs(fd))
    finally:
        s.close()


def test_fit_recovers_kappa_from_synthetic_data(small):
    from heatflow_amd.fit import fit_parameters

    cfg, stack, mesh = small
    exp = _synthetic_exp(cfg, mesh, ("p_sample",), [4.07])
    out = fit_parameters(cfg, None, ("p_sample",), exp, x0=[3.8], max_iter=40, backend=TangentOracleBackend(),
                         mesh=(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags))
    assert abs(out["values"][0] / 4.07 - 1) <= 1e-6, out["history"]
    assert out["converged"] and out["iterations"] <= 10 and out["rmse"] < 1e-8, out["history"]
    assert out["tangent_runs"] <= out["iterations"] + 1 < out["runs"]      # trials run the primal alone
    assert len(out["stderr"]) == 1


def test_fit_recovers_kappa_and_fwhm_jointly(small):
    from heatflow_amd.fit import fit_parameters

    cfg, stack, mesh = small
    exp = _synthetic_exp(cfg, mesh, ("p_sample", "fwhm"), [4.07, 1.2e-5])
    out = fit_parameters(cfg, None, ("p_sample", "fwhm"), exp, x0=[3.8, 1.32e-5], max_iter=20, backend=TangentOracleBackend(),
                         mesh=(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags))
    np.testing.assert_allclose(out["values"], [4.07, 1.2e-5], rtol=1e-5)


def test_run_tangent_rejects_a_tag_in_two_columns(small):
    from heatflow_amd.solver import HeatProblem

    cfg, stack, mesh = small
    from helpers import material_tables, reference_bcs

    bcs, ic, _ = reference_bcs(cfg, stack, mesh)
    k, rc = material_tables(stack, mesh)
    prob = HeatProblem(mesh.coords, mesh.tris, mesh.tags, k, rc, 1e-7, bcs, ic, backend=TangentOracleBackend())
    t = mesh.material_tags["p_sample"]
    with pytest.raises(ValueError):
        prob.run_tangent(2, [0], conductivity=[[t], [t]])
    with pytest.raises(ValueError):
        prob.run_tangent(2, [0])


def test_fit_cli_builds_the_mesh_and_writes_the_summary(tmp_path):
    """`python -m heatflow_amd.fit ... --output-dir DIR` on a fresh DIR: the mesh is built under DIR/mesh and
    fit_summary.json is written (the backend is the restated recursion)."""
    import json

    import yaml

    from conftest import load_cfg
    from heatflow_amd.fit import main
    from heatflow_amd.geometry import scale_mesh_sizes

    cfg = scale_mesh_sizes(load_cfg("geballe_with_diamond"), 8.0)
    cfg["timing"]["num_steps"] = 30
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    out_dir = tmp_path / "out"
    assert main(["--config", str(path), "--params", "p_sample", "--output-dir", str(out_dir), "--max-iter", "3"],
                backend=TangentOracleBackend()) == 0
    assert (out_dir / "mesh" / "mesh.msh").is_file() and (out_dir / "mesh" / "mesh_cfg.yaml").is_file()
    summary = json.loads((out_dir / "fit_summary.json").read_text())
    assert summary["params"] == ["p_sample"] and len(summary["values"]) == 1 and np.isfinite(summary["rmse"])
    assert summary["values"][0] > 0 and len(summary["stderr"]) == 1
    # a second call finds the mesh the first one built
    assert main(["--config", str(path), "--params", "p_sample", "--output-dir", str(out_dir), "--max-iter", "1"],
                backend=TangentOracleBackend()) == 0

