"""Derivatives of the region monitors in tangent runs, without a GPU: the restatement of
tests/monitor_tangent_oracle.py against central differences of the primal restatement and against hand values, combine_tangents
against central differences of combine, the Python-side errors, HeatProblem's call order, run_simulation end to end on the scipy
stand-in and the names of the C interface."""
import copy
import csv
import functools
import itertools
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import monitor_oracle as mo
import monitor_tangent_oracle as mto
from conftest import ROOT, build_case, load_cfg
from helpers import make_problem

from heatflow_amd import monitors as mon_mod

CASES = {"with_diamond": "geballe_with_diamond", "no_diamond": "geballe_no_diamond"}
EPS = mo.EPS


@functools.lru_cache(maxsize=None)
def small(which):
    return build_case(CASES[which], 8.0)


# ---- the restatement against central differences of the primal restatement --------------------------------------------------------------
def _smooth_fields(mesh):
    """A smooth state whose 350 .. 390 K contours cross the three layers radially, a smooth tangent of a few kelvin per unit of
    the parameter and a smooth z-velocity of the order of a nanometre per unit."""
    z, r = mesh.coords[:, 0], mesh.coords[:, 1]
    u = 300.0 + 200.0 * np.exp(-(r / 1.0e-5) ** 2) * (1.0 + 0.3 * np.sin(z * 1.0e6))
    t = 5.0 * np.cos(r / 8.0e-6) * (1.0 + 0.5 * np.cos(z * 7.0e5))
    v = 1.0e-9 * (0.3 + np.tanh(z * 6.0e5)) * (1.0 + 0.2 * np.cos(r / 6.0e-6))
    return u, t, v


@pytest.mark.parametrize("kind", ["field", "shape"])
@pytest.mark.parametrize("which", sorted(CASES))
def test_restatement_matches_central_differences_of_the_primal_restatement(which, kind):
    _, _, mesh = small(which)
    mt = mesh.material_tags
    th = {mt["p_sample"]: 380.0, mt["p_ins"]: 350.0, mt["p_coupler"]: 390.0}
    u, t, v = _smooth_fields(mesh)
    vel = v if kind == "shape" else None
    tags, tris = np.asarray(mesh.tags), np.asarray(mesh.tris)
    _, _, _, br = mo.per_tag(mesh.coords, tris, tags, u, th)
    steps = (4e-3, 2e-3, 1e-3)
    for tg, theta in th.items():
        assert np.all(br[tg] > 0), (tg, br[tg])                          # 0, 1, 2 and 3 nodes above: every branch
        uu = u[tris[tags == tg]]
        above = uu > theta
        cnt = above.sum(axis=1)
        cut = (cnt == 1) | (cnt == 2)
        odd = cnt == 1
        a = np.where(above[:, 0] == odd, 0, np.where(above[:, 1] == odd, 1, 2))
        rows = np.arange(len(uu))
        ua, ub, uc = uu[rows, a], uu[rows, (a + 1) % 3], uu[rows, (a + 2) % 3]
        assert min(np.abs(ua - ub)[cut].min(), np.abs(ua - uc)[cut].min()) >= 0.5      # every cut is well conditioned
        assert np.abs(uu - theta).min() > max(steps) * np.abs(t).max()   # no node crosses the threshold within the steps
    row, _, _ = mto.per_tag_tangent(mesh.coords, tris, tags, u, th, t[:, None], {0: vel} if vel is not None else None)
    err_h = {tg: [] for tg in th}
    for h in steps:
        sides = []
        for sg in (1.0, -1.0):
            c = np.array(mesh.coords, dtype=np.float64)
            if vel is not None:
                c[:, 0] += sg * h * vel
            rec, scale, _, b = mo.per_tag(c, tris, tags, u + sg * h * t, th)
            assert np.array_equal(b, br)                                 # the same branches on both sides
            sides.append((rec, scale))
        fd = (sides[0][0] - sides[1][0]) / (2.0 * h)
        for tg in th:
            # dI0 and dI1 are (bi)linear in the perturbation: the quotient is exact but for the rounding of the two sums it
            # subtracts.  A sum's own rounding is already half an ulp of sum_e |term_e| (all terms of I0 and I1 have one sign
            # here), so the "term" of the bound 8 eps max|term| / h is the tag's sum of |triangle terms| (monitor_oracle's scale),
            # the larger of the two sides - the largest single triangle could not bound a sum of a thousand of them.
            for f, name in ((0, "dI0"), (1, "dI1")):
                bound = 8.0 * EPS * max(sides[0][1][tg, f], sides[1][1][tg, f]) / h
                err = abs(fd[tg, 4 + f] - row[tg, 0, 2 + f])
                assert err <= bound, (kind, h, tg, name, err, bound)
            err_h[tg].append(abs(fd[tg, 6] - row[tg, 0, 4]))
        if vel is None:
            assert np.all(row[:, 0, 2] == 0.0)
    for tg, e in err_h.items():
        print(f"{which} {kind} tag {tg}: dH = {row[tg, 0, 4]:.6e}, |FD - dH| at h = 4e-3, 2e-3, 1e-3: {e[0]:.3e} {e[1]:.3e} {e[2]:.3e} "
              f"(factors {e[0] / e[1]:.3f}, {e[1] / e[2]:.3f})")
        assert row[tg, 0, 4] != 0.0
        for big, half in ((e[0], e[1]), (e[1], e[2])):                   # second order: the error falls by 4 per halving
            assert 3.5 <= big / half <= 4.5, (tg, e)


# ---- every branch of dH on one triangle, by hand --------------------------------------------------------------------------------------------
def test_every_branch_of_dH_on_one_triangle_in_every_vertex_order():
    """The right triangle of test_monitors_cpu (legs 1, r in [1, 2]) with u = z: H(c) = int over {z > c} of r dA = strip(c).
    A tangent t shifts the cut: t = 1 lowers the threshold (dH = the line integral of r along the cut, ((2 - c)^2 - 1) / 2), t = z
    scales u (dH = c times that), t = r tilts the cut (dH = int r^2 dr along it, ((2 - c)^3 - 1) / 3).  A velocity v = z stretches
    the triangle along z with the nodal values kept: every integral grows with the area, q = 1."""
    coords = np.array([[0.0, 1.0], [1.0, 1.0], [0.0, 2.0]])
    z, r = coords[:, 0], coords[:, 1]
    c = 0.25
    line = ((2.0 - c) ** 2 - 1.0) / 2.0
    strip = lambda x: (-(2.0 - 1.0) ** 3 / 6.0 - 0.5) - (-(2.0 - x) ** 3 / 6.0 - 0.5 * x)      # noqa: E731
    for perm in itertools.permutations(range(3)):                        # three rotations in both orientations
        tri = np.array([list(perm)])
        for u, theta, cnt, sign in ((z, c, 1, 1.0), (-z, -c, 2, -1.0)):  # one node above (z > c); two above (z < c)
            for t, want in ((np.ones(3), line), (sign * z, sign * c * line), (r, ((2.0 - c) ** 3 - 1.0) / 3.0)):
                (dI0, dI1, dH), _, n = mto.triangle_tangent_terms(coords, tri, u, theta, t)
                assert n[0] == cnt and dI0[0] == 0.0
                assert abs(dH[0] - want) <= 4e-15, (perm, cnt, dH[0], want)
            (dI0, dI1, dH), _, _ = mto.triangle_tangent_terms(coords, tri, u, theta, np.zeros(3), v=z)
            H = strip(c) if cnt == 1 else strip(0.0) - strip(c)
            assert abs(dI0[0] - strip(0.0)) <= 4e-15 and abs(dI1[0] - sign * 5.0 / 24.0) <= 4e-15 and abs(dH[0] - H) <= 4e-15
            # a rigid shift along z changes nothing
            (dI0, dI1, dH), _, _ = mto.triangle_tangent_terms(coords, tri, u, theta, np.zeros(3), v=np.full(3, 0.7))
            assert dI0[0] == 0.0 and dI1[0] == 0.0 and dH[0] == 0.0
        for theta, cnt in ((-1.0, 3), (1.5, 0)):                         # all above, none above: dH = 0 whatever the tangent
            (dI0, dI1, dH), _, n = mto.triangle_tangent_terms(coords, tri, z, theta, r)
            assert n[0] == cnt and dH[0] == 0.0
        # dI1 of t = r: int r^2 dA = int_0^1 ((2 - z)^3 - 1) / 3 dz = 11 / 12
        (dI0, dI1, dH), _, _ = mto.triangle_tangent_terms(coords, tri, z, 5.0, r)
        assert abs(dI1[0] - 11.0 / 12.0) <= 4e-15


# ---- combine_tangents against central differences of combine ---------------------------------------------------------------------------------
def _records(K, tab_len, n_par, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros((K, tab_len, 7))
    rec[:, :, 0] = 400.0 + 100.0 * rng.random((K, tab_len))
    rec[:, :, 2] = 300.0 + 50.0 * rng.random((K, tab_len))
    rec[:, :, 1] = rng.integers(0, 50, (K, tab_len))
    rec[:, :, 3] = rng.integers(0, 50, (K, tab_len))
    rec[:, :, 4] = 1.0e-16 * (1.0 + rng.random((K, tab_len)))
    rec[:, :, 5] = rec[:, :, 4] * (320.0 + 60.0 * rng.random((K, tab_len)))
    rec[:, :, 6] = rec[:, :, 4] * rng.random((K, tab_len))
    drec = rng.standard_normal((K, tab_len, n_par, 5))
    drec[:, :, :, 2:] *= rec[:, :, None, 4:5] * np.array([0.05, 20.0, 0.3])
    return rec, drec


def _moved(rec, drec, j, h):
    out = rec.copy()
    out[:, :, 0] += h * drec[:, :, j, 0]
    out[:, :, 2] += h * drec[:, :, j, 1]
    out[:, :, 4:] += h * drec[:, :, j, 2:]
    return out


def test_combine_tangents_matches_central_differences_of_combine():
    K, tab_len, n_par = 6, 8, 3
    rec, drec = _records(K, tab_len, n_par, 1)
    # the pair's peak sits in tag 3 in the even records and in tag 4 in the odd ones; its minimum the other way round
    rec[0::2, 3, 0], rec[0::2, 4, 0] = 520.0, 510.0
    rec[1::2, 3, 0], rec[1::2, 4, 0] = 505.0, 515.0
    rec[0::2, 3, 2], rec[0::2, 4, 2] = 301.0, 290.0
    rec[1::2, 3, 2], rec[1::2, 4, 2] = 291.0, 302.0
    regions = {"sample": {"tags": [4], "above": 380.0}, "pair": {"tags": [3, 4], "above": None}, "hot": {"tags": [2, 3], "above": 350.0}}
    rho_c = {2: 1.5e6, 3: 2.5e6, 4: 3.0e6}
    T_ref, coords = 300.0, np.zeros((50, 2))
    cap = {4: 1, 3: 2}                                                   # column 1 carries the rho_c of tag 4, column 2 the one of tag 3
    got = mon_mod.combine_tangents(rec, drec, regions, rho_c=rho_c, T_ref=T_ref, capacity_columns=cap)
    assert set(got) == set(regions) and set(got["pair"]) == {"T_max", "T_min", "volume", "T_mean", "energy"}
    assert set(got["sample"]) == set(mon_mod.TANGENT_FIELDS)
    h = 1e-6
    for j in range(n_par):
        sides = []
        for sg in (1.0, -1.0):
            rc = {t: v + (sg * h if cap.get(t) == j else 0.0) for t, v in rho_c.items()}
            sides.append(mon_mod.combine(_moved(rec, drec, j, sg * h), regions, coords, rho_c=rc, T_ref=T_ref))
        for region in regions:
            for field, d in got[region].items():
                fd = (sides[0][region][field] - sides[1][region][field]) / (2.0 * h)
                # combine is rational in the records: the quotient's error is h^2 times third derivatives plus eps / h of the
                # values, both far below 1e-7 of the derivative's size here
                assert np.max(np.abs(d[:, j] - fd)) <= 1e-7 * max(np.max(np.abs(d[:, j])), np.max(np.abs(fd))), (j, region, field)
    # the peak's derivative is the one of the tag that holds it
    assert np.array_equal(got["pair"]["T_max"][0::2], drec[0::2, 3, :, 0]) and np.array_equal(got["pair"]["T_max"][1::2], drec[1::2, 4, :, 0])
    assert np.array_equal(got["pair"]["T_min"][0::2], drec[0::2, 4, :, 1]) and np.array_equal(got["pair"]["T_min"][1::2], drec[1::2, 3, :, 1])
    # equal peaks: combine's tie rule, the lowest tag
    tie = rec.copy()
    tie[:, 4, 0] = tie[:, 3, 0]
    assert np.array_equal(mon_mod.combine_tangents(tie, drec, regions)["pair"]["T_max"], drec[:, 3, :, 0])
    # cv and rho: the whole column is scaled, the explicit term included - against central differences in cv
    rho, cv = 2000.0, 1500.0
    rho_c[4] = rho * cv
    scaled = mon_mod.combine_tangents(rec, drec, regions, rho_c=rho_c, T_ref=T_ref, capacity_columns={4: 1}, scale=[1.0, rho, 1.0])
    sides = [mon_mod.combine(_moved(rec, drec, 1, sg * h * rho), regions, coords, rho_c={**rho_c, 4: rho * (cv + sg * h)}, T_ref=T_ref)
             for sg in (1.0, -1.0)]
    for region in ("sample", "pair"):
        for field in ("energy", "T_mean", "T_max"):
            fd = (sides[0][region][field] - sides[1][region][field]) / (2.0 * h)
            assert np.max(np.abs(scaled[region][field][:, 1] - fd)) <= 1e-7 * np.max(np.abs(fd)), (region, field)
    plain = mon_mod.combine_tangents(rec, drec, regions, rho_c=rho_c, T_ref=T_ref, capacity_columns={4: 1})
    assert np.array_equal(scaled["pair"]["energy"][:, 0], plain["pair"]["energy"][:, 0])
    # energy is left out wherever combine leaves it out: a capacity table on a tag, a tag without a constant, no constants at all
    assert "energy" not in mon_mod.combine_tangents(rec, drec, regions, rho_c=rho_c, T_ref=T_ref, tabled={4})["sample"]
    assert "energy" in mon_mod.combine_tangents(rec, drec, regions, rho_c=rho_c, T_ref=T_ref, tabled={4})["hot"]
    assert "energy" not in mon_mod.combine_tangents(rec, drec, regions, rho_c={4: 1.0}, T_ref=T_ref)["pair"]
    assert "energy" not in mon_mod.combine_tangents(rec, drec, regions)["sample"]
    one = mon_mod.combine_tangents(rec[0], drec[0], regions)             # a single record
    assert one["sample"]["T_mean"].shape == (1, n_par)
    with pytest.raises(ValueError, match="combine_tangents: records .* do not belong together"):
        mon_mod.combine_tangents(rec[:2], drec[:3], regions)


def test_uncertainty_is_the_root_sum_of_squares():
    d = {"a": {"sample": {"T_mean": np.array([3.0, 0.0])}}, "b": {"sample": {"T_mean": np.array([2.0, 1.0])}}}
    band = mon_mod.uncertainty(d, {"a": 1.0, "b": 2.0})
    assert np.allclose(band["sample"]["T_mean"], [5.0, 2.0])
    assert mon_mod.check_sigma({"p_sample.rho_c": "0.15"}) == {"p_sample.rho_c": 0.15}
    for bad, pat in (({"fwhm": 0.0}, "monitor_sigma: fwhm: .*positive and finite"), ({"fwhm": -0.1}, "monitor_sigma: fwhm"),
                     ({"fwhm": math.inf}, "monitor_sigma: fwhm"), ({"fwhm": math.nan}, "monitor_sigma: fwhm"),
                     ({"fwhm": "x"}, "monitor_sigma: fwhm: a number is expected"), ({}, "monitor_sigma must be a mapping"),
                     ([("fwhm", 0.1)], "monitor_sigma must be a mapping")):
        with pytest.raises(ValueError, match=pat):
            mon_mod.check_sigma(bad)


# ---- HeatProblem ---------------------------------------------------------------------------------------------------------------------------
class RecordingBackend:
    """Records the HeatflowHIP calls HeatProblem makes; tangent runs return arrays of the right shapes."""
    tangent_nv = 2

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def rec(*a, **k):
            self.calls.append(name)
            if name == "run_tangent":
                n = len(a[0])
                return np.zeros((n, 0)), np.zeros(n, dtype=np.int32), np.zeros((n, 2, 0)), np.zeros((n, 2), dtype=np.int32)
            if name == "monitor_tangent_count":
                return 4, 2
            if name == "get_monitor_tangents":
                return np.zeros((3, 8, 2, 5)), np.array([5, 6, 7], dtype=np.int32)
            if name == "get_monitors":
                return np.ones((8, 8, 7))
            return None
        return rec


def test_heat_problem_call_order_with_and_without_monitor_tangents():
    cfg, stack, mesh = small("with_diamond")
    regions = {"sample": {"tags": [4], "above": 2000.0}, "pair": {"tags": [3, 4]}}
    be = RecordingBackend()
    prob = make_problem(cfg, stack, mesh, backend=be, monitors=regions)
    n0 = len(be.calls)
    prob.run_tangent(3, None, conductivity=[[4]], capacity=[[], [4]])
    assert be.calls[n0:] == ["tangent_setup", "tangent_set_capacity", "run_tangent"]      # the default: no new call
    n1 = len(be.calls)
    prob.run_tangent(3, None, conductivity=[[4]], capacity=[[], [4]], monitor_tangents=True)
    assert be.calls[n1:] == ["monitor_tangent_count", "set_monitor_tangents", "run_tangent", "set_monitor_tangents"]
    n2 = len(be.calls)
    hist = prob.monitor_tangent_history()
    assert be.calls[n2:] == ["get_monitor_tangents", "get_monitors"]
    assert set(hist) == {"sample", "pair"} and hist["pair"]["T_mean"].shape == (3, 2) and "hot_volume" not in hist["pair"]
    # the problem remembers the run's capacity columns: the explicit term of energy sits in column 1 alone (records of ones,
    # derivative records of zeros: 2 pi (I1 - T_ref I0) = 2 pi (1 - 300))
    assert np.all(hist["sample"]["energy"][:, 0] == 0.0) and np.allclose(hist["sample"]["energy"][:, 1], 2.0 * math.pi * (1.0 - 300.0))
    n3 = len(be.calls)
    prob.run_tangent(2, None, conductivity=[[4]], capacity=[[], [4]])
    assert be.calls[n3:] == ["run_tangent"]
    plain = RecordingBackend()
    p2 = make_problem(cfg, stack, mesh, backend=plain)
    n = len(plain.calls)
    with pytest.raises(ValueError, match="run_tangent: monitor_tangents needs monitors"):
        p2.run_tangent(3, None, conductivity=[[4]], monitor_tangents=True)
    with pytest.raises(ValueError, match="monitors: the problem has no monitors"):
        p2.monitor_tangent_history()
    assert plain.calls[n:] == []
    p3 = make_problem(cfg, stack, mesh, backend=RecordingBackend(), monitors=regions)
    with pytest.raises(ValueError, match="monitor_tangents: no tangent run with monitor_tangents=True yet"):
        p3.monitor_tangent_history()


# ---- the drivers -------------------------------------------------------------------------------------------------------------------------------
NSTEPS, T_FINAL, MONITORS = mto.FD_NSTEPS, mto.FD_T_FINAL, mto.FD_MONITORS
FD_REL_STEP, FD_FLOAT64, FD_TOL = mto.FD_REL_STEP, mto.FD_FLOAT64, mto.FD_TOL
FD_FIELDS = ("T_mean", "energy", "T_max")


def _cfg(which="with_diamond", block=MONITORS, nsteps=NSTEPS):
    cfg = copy.deepcopy(small(which)[0])
    cfg["timing"] = dict(cfg["timing"], num_steps=nsteps, t_final=T_FINAL)
    if block is not None:
        cfg["monitors"] = copy.deepcopy(block)
    return cfg


def _session(mesh):
    from heatflow_amd.driver import SimulationSession

    return SimulationSession(mesh.coords, mesh.tris, mesh.tags, mesh.material_tags, backend=mto.MonitorTangentOracleBackend(), precond=0)


def _moved_run(cfg, mesh, name, value):
    """The monitors of a stand-in run with ``name`` set to ``value`` (a thickness moves the nodes; the triangles stay)."""
    from heatflow_amd.fit import get_param, set_params
    from heatflow_amd.geometry import build_stack, thickness_velocity
    from heatflow_amd.parameter_sweep import get_watcher_points

    c = set_params(cfg, (name,), (value,))
    m = mesh
    if name.endswith(".thickness"):
        coords = np.array(mesh.coords, dtype=np.float64)
        coords[:, 0] += thickness_velocity(cfg, name.rsplit(".", 1)[0], mesh.coords[:, 0]) * (value - get_param(cfg, name))
        m = SimpleNamespace(coords=coords, tris=mesh.tris, tags=mesh.tags, material_tags=mesh.material_tags)
    s = _session(m)
    try:
        res = s.run(c, build_stack(c), None)
        return res["monitors"], s.problem.backend.get_monitors()
    finally:
        s.close()


def fd_errors(cfg, mesh, name, rel, derivs, base_records):
    """{(region, field): max over the steps of |derivative - central difference| / max |derivative|}; asserts that the peak's
    node is the same in the three runs."""
    from heatflow_amd.fit import get_param

    t0 = get_param(cfg, name)
    (mp, rp), (mm, rm) = (_moved_run(cfg, mesh, name, t0 * (1.0 + sg * rel)) for sg in (1.0, -1.0))
    assert np.array_equal(rp[:, :, 1], base_records[:, :, 1]) and np.array_equal(rm[:, :, 1], base_records[:, :, 1])
    out = {}
    for region in derivs:
        for field in FD_FIELDS:
            d = derivs[region][field]
            fd = (mp[region][field] - mm[region][field]) / (2.0 * rel * t0)
            out[(region, field)] = float(np.max(np.abs(d - fd)) / np.max(np.abs(d)))
    return out


@pytest.mark.parametrize("which", sorted(CASES))
def test_run_simulation_writes_the_bands_and_the_derivatives_match_central_differences(which, tmp_path):
    import importlib

    from heatflow_amd.fit import get_param
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small(which)
    cfg = _cfg(which)
    names = list(FD_REL_STEP)
    sigma = {"p_sample.rho_c": 0.15, "p_sample.thickness": 0.05, "fwhm": 0.1}
    mod = importlib.import_module("heatflow_amd.run_" + which)
    s = _session(mesh)
    try:
        out = tmp_path / "out"
        res = mod.run_simulation(cfg, str(tmp_path / "mesh"), output_folder=str(out), session=s, tangents=["p_sample"],
                                 monitor_sigma=sigma, watcher_points=get_watcher_points(cfg), write_xdmf=False, suppress_print=True,
                                 read_flux=False)
        base_records = s.problem.backend.get_monitors()
    finally:
        s.close()
    params = ["p_sample", "p_sample.rho_c", "p_sample.thickness", "fwhm"]      # tangents first, then the names of monitor_sigma
    assert list(res["monitor_tangents"]) == params and list(res["tangents"]) == params
    mt, band, m = res["monitor_tangents"], res["monitor_uncertainty"], res["monitors"]
    assert list(band) == ["sample", "coupler"] and "hot_fraction" in band["sample"] and "hot_fraction" not in band["coupler"]
    assert all(len(v) == NSTEPS for f in band.values() for v in f.values())
    assert m["sample"]["hot_fraction"].max() > 0.0 and band["sample"]["hot_fraction"].max() > 0.0
    # the band is the root sum of squares over the names of monitor_sigma (the k column is no part of it)
    for region in band:
        for field in band[region]:
            want = np.sqrt(sum((mt[q][region][field] * sg * get_param(cfg, q)) ** 2 for q, sg in sigma.items()))
            assert np.allclose(band[region][field], want, rtol=1e-14, atol=0.0), (region, field)
    # monitor_uncertainty.csv: time, <region>.<field>, <region>.<field>.sigma; monitors.csv keeps its columns
    with open(out / "monitor_uncertainty.csv", newline="") as f:
        rows = list(csv.reader(f))
    with open(out / "monitors.csv", newline="") as f:
        mrows = list(csv.reader(f))
    assert mrows[0] == ["time"] + [f"{r}.{f}" for r, f in mon_mod.csv_columns(m)]
    assert [r[0] for r in rows[1:]] == [r[0] for r in mrows[1:]] and len(rows) == NSTEPS + 1
    head = rows[0][1:]
    assert head[0::2] == [f"{r}.{f}" for r, f in mon_mod.csv_columns(m) if f in band[r]] and head[1::2] == [c + ".sigma" for c in head[0::2]]
    for j, col in enumerate(rows[0][1:], start=1):
        region, field = col.split(".")[:2]
        src = band if col.endswith(".sigma") else m
        assert [float(r[j]) for r in rows[1:]] == np.asarray(src[region][field]).tolist(), col
    # the derivatives against central differences of two stand-in runs
    for name in names:
        rel = FD_REL_STEP[name]
        errs = fd_errors(cfg, mesh, name, rel, mt[name], base_records)
        worst = max(errs.values())
        print(f"{which} {name}: relative step {rel:g}, |derivative - central difference| / max|derivative|: "
              + ", ".join(f"{r}.{f} {e:.2e}" for (r, f), e in errs.items()))
        assert worst <= 0.25 * FD_TOL, "the step recorded in FD_REL_STEP is the one the rule finds"
        assert FD_TOL >= 10.0 * FD_FLOAT64[name] and worst <= 4.0 * FD_FLOAT64[name], (name, worst)
        assert worst <= FD_TOL


def test_python_errors_name_their_argument(tmp_path):
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.parameter_sweep import get_watcher_points

    _, _, mesh = small("with_diamond")
    cfg = _cfg()
    stack, wp = build_stack(cfg), get_watcher_points(cfg)
    plain = _cfg(block=None)
    s = _session(mesh)
    try:
        with pytest.raises(ValueError, match="monitor_tangents: the configuration has no monitors block"):
            s.run(plain, stack, wp, tangents=["p_sample"], monitor_tangents=True)
        with pytest.raises(ValueError, match="monitor_sigma: the configuration has no monitors block"):
            s.run(plain, stack, wp, monitor_sigma={"fwhm": 0.1})
        with pytest.raises(ValueError, match="monitor_tangents: no parameter"):
            s.run(cfg, stack, wp, monitor_tangents=True)
        for bad in (0.0, -0.1, math.inf, math.nan):
            with pytest.raises(ValueError, match="monitor_sigma: fwhm: the relative one-sigma must be positive and finite"):
                s.run(cfg, stack, wp, monitor_sigma={"fwhm": bad})
        mats = [m for m in cfg["mats"]]
        many = {m: 0.1 for m in mats} | {f"{m}.rho_c": 0.1 for m in mats}
        with pytest.raises(ValueError, match=r"monitor_sigma: 18 tangent columns \(at most 16 per run\)"):
            s.run(cfg, stack, wp, monitor_sigma=many)
        with pytest.raises(ValueError, match=r"monitor_tangents: 17 tangent columns"):
            s.run(cfg, stack, wp, tangents=list(many)[:17], monitor_tangents=True)
        with pytest.raises(ValueError, match="tangents: unknown parameter 'nothing.k_q'|tangents: .*nothing"):
            s.run(cfg, stack, wp, monitor_sigma={"nothing.k_q": 0.1})
        # what tangents= refuses stays refused, with the messages of before
        with pytest.raises(ValueError, match="tangents: not combined with a field sink or the read-flux projection"):
            s.run(cfg, stack, wp, monitor_sigma={"fwhm": 0.1}, field_sink=lambda t, u: None)
        with pytest.raises(ValueError, match="tangents: not combined with a field sink or the read-flux projection"):
            s.run(cfg, stack, wp, monitor_sigma={"fwhm": 0.1}, read_flux=True)
        for base, pat in (("geballe_with_diamond_source", "tangents="), ("geballe_with_diamond_kT", "tangents"),
                          ("geballe_with_diamond_cvT", "tangents")):
            c = copy.deepcopy(load_cfg(base))
            c["mats"] = {k: dict(v, mesh=float(v["mesh"]) * 8.0) for k, v in c["mats"].items()}
            c["monitors"] = copy.deepcopy(MONITORS)
            for kw in ({"monitor_sigma": {"p_sample": 0.1}}, {"tangents": ["p_sample"], "monitor_tangents": True}):
                with pytest.raises(ValueError, match=pat):
                    s.run(c, build_stack(c), get_watcher_points(c), **kw)
    finally:
        s.close()


def test_cli_takes_monitor_sigma(tmp_path, monkeypatch):
    import yaml

    from heatflow_amd import driver

    cfg_path = tmp_path / "cfg.yaml"
    with open(cfg_path, "w") as f:
        yaml.safe_dump(_cfg(), f)
    seen = {}
    monkeypatch.setattr(driver, "run_simulation_impl", lambda *a, **k: seen.update(k))
    assert driver.cli("with_diamond", ["--config", str(cfg_path), "--monitor-sigma", "p_sample.rho_c=0.15", "fwhm=0.1"]) == 0
    assert seen["monitor_sigma"] == {"p_sample.rho_c": 0.15, "fwhm": 0.1}
    seen.clear()
    assert driver.cli("with_diamond", ["--config", str(cfg_path)]) == 0 and "monitor_sigma" not in seen
    for bad in ("fwhm", "fwhm=x", "=0.1"):
        with pytest.raises(SystemExit):
            driver.cli("with_diamond", ["--config", str(cfg_path), "--monitor-sigma", bad])


# ---- the C interface ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_backend_lists_the_entry_points():
    from heatflow_amd import hip_backend

    with open(os.path.join(ROOT, "include", "heatflow_hip.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = re.findall(r"\b(hf_\w+)\s*\(", text)
    assert len(declared) == len(set(declared)) and sorted(declared) == sorted(hip_backend.EXPORTS)      # name for name
    with open(os.path.join(ROOT, "heatflow_amd", "csrc", "heatflow_hip.hip")) as f:
        impl = f.read()
    for name in ("hf_set_monitor_tangents", "hf_monitor_tangent_count", "hf_get_monitor_tangents", "hf_monitor_tangent_eval"):
        assert name in declared and re.search(rf"^int {name}\(", impl, flags=re.M)
    assert re.search(r"int\s+hf_get_monitor_tangents\(hf_ctx\*\s*ctx,\s*int32_t\s+first,\s*int32_t\s+count,\s*double\*\s*out,\s*int32_t\*\s*record_index",
                     text)
    assert re.search(r"int\s+hf_monitor_tangent_eval\(hf_ctx\*\s*ctx,\s*int32_t\s+nv,\s*const double\*\s*s,\s*int32_t\s+n_shape,\s*"
                     r"const int32_t\*\s*shape_col,\s*const double\*\s*vz,\s*double\*\s*out\);", text)
    for method in ("set_monitor_tangents", "monitor_tangent_count", "get_monitor_tangents", "monitor_tangent_eval"):
        assert callable(getattr(hip_backend.HeatflowHIP, method))
