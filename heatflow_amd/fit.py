"""Least-squares fit of material parameters to a measured o-side curve, on tangent runs.

The objective is the kappa sweep's (parameter_sweep.oside_rmse, sweep_test.py:76-93): the simulated o-side rise
(o - o[0]) / (p.max - p.min), interpolated onto the experimental times, against the experiment's normalised o-side curve.
Instead of a grid, Levenberg-Marquardt steps in log(theta) (theta stays positive) on the residuals r_i, with the Jacobian
from one tangent run per accepted iterate (HeatProblem.run_tangent): the derivative of the normalised curve is chain-ruled through
the normalisation with the p-side's argmax and argmin held fixed.  A trial step costs one primal run; the tangents run
only at accepted iterates.  Standard errors come from s^2 (J^T J)^-1, s^2 = sum r^2 / (m - p).

    python -m heatflow_amd.fit --config cfgs/geballe_with_diamond.yaml --params p_sample [fwhm] --output-dir DIR
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import time

import numpy as np

from .geometry import check_thickness_name, thickness_velocity
from .parameter_sweep import build_stack, get_watcher_points, oside_curves
from .aniso import (CAPACITY_KINDS, DIRECTIONAL_HINT, KEY, PARAM_KINDS, check_capacity_names, classify_param, material_aniso,
                    refuse_aniso, refuse_aniso_tables)
from .stepping import refuse_variable_steps
from .kappa_t import (check_table_tangents, refuse_enthalpy, get_table_param, refuse_tables, set_table_param, table_keys,
                      table_tangents)
from .source import check_source_param, parse_source, refuse_source_tangents
from .monitors import refuse_monitors

DEFAULT_EXP_CSV = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "experimental_data",
                               "geballe_heat_data.csv")


def _resolve_param(cfg, name):
    """(kind, material name, what carries it) of a parameter name, the kind and the name from aniso.classify_param: the material's
    block of ``cfg``, the validated source for a "source.*" name, None for "fwhm".  ValueError naming the parameter for an unknown
    material or suffix, a table name on a material without that block, and a source name the source does not have."""
    kind, mat = classify_param(name)
    if kind == "fwhm":
        return kind, mat, None
    if kind == "source":
        spec = parse_source(cfg)
        check_source_param(spec, name)
        return kind, mat, spec
    if kind == "table":
        get_table_param(cfg, name)       # (an unknown material or a missing block: ValueError)
    elif mat not in cfg["mats"]:
        raise ValueError(f"parameter {name!r}: no material {mat!r} in the configuration")
    return kind, mat, cfg["mats"][mat]


def get_param(cfg, name):
    """The value of a parameter: "fwhm", a material's k ("<m>" or "<m>.k"), its directional conductivity "<m>.k_r" =
    k * k_aniso.r / "<m>.k_z" = k * k_aniso.z in W/m/K (multiplier 1 where the block or the key is absent), or its layer
    thickness "<m>.thickness" = mats.<m>.z in metres (the materials whose z the stack reads), or its heat capacity: "<m>.rho_c" =
    rho * cv in J/m^3/K, "<m>.cv", "<m>.rho"; or a parameter of the volumetric source: "source.power" in W,
    "source.fwhm" (the beam's width, heating.fwhm where the block has none) and "source.depth" in metres, "source.pulse.t0" and
    "source.pulse.fwhm" of a Gaussian pulse in seconds."""
    kind, mat, block = _resolve_param(cfg, name)
    if kind == "fwhm":
        return float(cfg["heating"]["fwhm"])
    if kind == "source":
        if name.startswith("source.pulse."):
            return float(block.pulse[1 if name.endswith(".t0") else 2])
        return float({"source.power": block.power, "source.fwhm": block.fwhm, "source.depth": block.depth}[name])
    if kind == "table":      # "<m>.k_power.exponent", "<m>.cv_einstein.theta", or a table's scale (1 as it stands)
        return get_table_param(cfg, name)
    if kind == "k":
        return float(block["k"])
    if kind == "thickness":
        check_thickness_name(cfg, mat, name)
        return float(block["z"])
    if kind in CAPACITY_KINDS:
        return float(block["rho"]) * float(block["cv"]) if kind == "rho_c" else float(block[kind])
    m = material_aniso(mat, block) or (1.0, 1.0)
    return float(block["k"]) * m[0 if kind == "k_r" else 1]


def set_params(cfg, params, values):
    """A copy of ``cfg`` with the parameters set: "fwhm" of the heating profile, the conductivity k of a material ("<m>" or
    "<m>.k"; the multipliers of a ``k_aniso`` block stay), or a directional conductivity: "<m>.k_r" writes k_aniso.r = value / k,
    "<m>.k_z" k_aniso.z, creating the block where absent; "<m>.thickness" writes mats.<m>.z in metres; "<m>.rho_c"
    writes cv = value / rho and keeps rho, "<m>.cv" and "<m>.rho" write their key (two of the three on one material: ValueError); a source parameter writes its key of ``heating.source``
    ("source.fwhm" writes heating.source.fwhm explicitly, whether the block had one or took heating.fwhm).  The k parameters are applied first, so a directional value holds
    whatever the order of the names."""
    c = copy.deepcopy(cfg)
    check_capacity_names(params)
    directional = []
    for name, v in zip(params, values):
        kind, mat, block = _resolve_param(c, name)
        if kind == "fwhm":
            c["heating"]["fwhm"] = float(v)
        elif kind == "source":
            block = c["heating"]["source"]
            if name.startswith("source.pulse."):
                block["pulse"][name.rsplit(".", 1)[1]] = float(v)
            else:
                block[name.split(".", 1)[1]] = float(v)
        elif kind == "table":
            set_table_param(c, name, v)
        elif kind == "k":
            block["k"] = float(v)
        elif kind == "thickness":
            check_thickness_name(c, mat, name)
            block["z"] = float(v)
        elif kind == "rho_c":
            block["cv"] = float(v) / float(block["rho"])
        elif kind in CAPACITY_KINDS:
            block[kind] = float(v)
        else:
            directional.append((block, PARAM_KINDS[kind], v))
    for block, direction, v in directional:
        block.setdefault(KEY, {})[direction] = float(v) / float(block["k"])
    return c


def load_experiment(exp_csv):
    """The experiment's columns (time, temp, oside): a CSV path, or a structured array / dict already loaded."""
    if isinstance(exp_csv, (str, os.PathLike)):
        return np.genfromtxt(exp_csv, delimiter=",", names=True)
    return exp_csv


def residual_and_jacobian(res, params, exp, ic_temp):
    """Residuals r = exp curve - sim curve on the experimental times and dr/dtheta (m x p) of one tangent run's result
    (Session.run(..., tangents=params)).  The normalisation's argmax / argmin of the p-side curve are held fixed."""
    ps, os_ = res["watchers"]["pside"], res["watchers"]["oside"]
    t_exp, y_exp, t_sim, y_sim = oside_curves(exp, ic_temp, res["times"], ps, os_)
    r = y_exp - np.interp(t_exp, t_sim, y_sim)
    imax, imin = int(np.argmax(ps)), int(np.argmin(ps))
    span = ps[imax] - ps[imin]
    J = np.empty((len(r), len(params)))
    for j, p in enumerate(params):
        dp, do = res["tangents"][p]["pside"], res["tangents"][p]["oside"]
        dy = (do - do[0]) / span - (os_ - os_[0]) * (dp[imax] - dp[imin]) / span ** 2
        J[:, j] = -np.interp(t_exp, t_sim, dy)        # interpolation is linear in the values
    return r, J


def fit_parameters(cfg, mesh_folder, params=("p_sample",), exp_csv=DEFAULT_EXP_CSV, x0=None, max_iter=20, *, xtol=1e-9,
                   ftol=1e-10, session=None, backend=None, device_id=0, rtol=1e-10, mesh=None, rebuild_mesh=None,
                   verbose=False, nuisance=None):
    """Levenberg-Marquardt fit of ``params`` (material names, "<material>.k_r" / "<material>.k_z" / "<material>.k" /
    "<material>.thickness" / "<material>.rho_c" / "<material>.cv" / "<material>.rho" - see :func:`get_param` - and / or "fwhm") to the experiment's o-side curve.  With a thickness among
    them the mesh (``mesh`` / ``mesh_folder`` / the session's) is taken as that of ``cfg``; its triangles stay and its nodes move
    with the trial thicknesses, so the fitted run lives on a deformed mesh (``deformed_mesh`` of the result).
    ``x0`` = start values (default: the configuration's).  ``session`` / ``backend`` / ``mesh`` = (coords, tris, tags,
    tag_map) reuse what the caller has; otherwise the mesh is loaded from ``mesh_folder``, or built there (``rebuild_mesh``
    True, or None and the folder holds no mesh).  A trial step costs one primal run; only an accepted step is followed by a
    tangent run for the next Jacobian.  Returns {params, values, rmse, converged, iterations, history, stderr, runs,
    tangent_runs, seconds, scheme}.  The time scheme is the configuration's (``timing.scheme``, default backward Euler);
    the tangents are those of the discrete loop of that scheme.
    ``nuisance`` = {name: relative sigma} adds a systematic-error budget: the names are parameters the fit accepts
    that are not among ``params`` (assumed capacities, thicknesses, the beam width, other conductivities), sigma their relative
    one-sigma uncertainty.  After convergence one more tangent run at the fitted values carries the columns params + nuisance; with
    J the Jacobian of the fitted parameters and J_q the column of nuisance q, a nuisance that is off by sigma_q moves the fit by
    d theta_q = -(J^T J)^-1 J^T J_q (sigma_q value_q).  The result gains ``systematic`` {nuisance: {param: shift}} and
    ``systematic_total`` {param: root sum of squares over the nuisances}, next to ``stderr``."""
    from .driver import SimulationSession, prepare_mesh, time_scheme

    t0 = time.time()
    scheme = time_scheme(cfg)
    refuse_enthalpy(cfg, "heatflow_amd.fit")
    refuse_variable_steps(cfg, "heatflow_amd.fit")
    refuse_aniso_tables(cfg, "heatflow_amd.fit")     # both kinds: forward runs only, with timing.table_tangents too
    tab_on = table_tangents(cfg) and bool(table_keys(cfg))      # timing.table_tangents
    if tab_on:
        check_table_tangents(cfg, "heatflow_amd.fit", tuple(params) + tuple(nuisance or ()))
    else:
        refuse_tables(cfg, "heatflow_amd.fit")
    refuse_source_tangents(cfg, "heatflow_amd.fit")     # a source fits only under heating.source.tangents: true
    refuse_monitors(cfg, "heatflow_amd.fit")
    params = tuple(params)
    refuse_aniso(cfg, "heatflow_amd.fit of the conductivity of an anisotropic material", set(params), DIRECTIONAL_HINT)
    for p in params:
        if p == "source.power":
            raise ValueError("parameter 'source.power' cannot be fitted: the objective is normalised by the p-side span and the "
                             "temperature rise is linear in the power, so its Jacobian column is identically zero (it is valid "
                             "as a nuisance, in tangents= and in monitor_sigma=)")
        _resolve_param(cfg, p)           # an unknown material or suffix, before any mesh or session is made
    nuisance = {str(q): v for q, v in dict(nuisance or {}).items()}
    for q, sig in nuisance.items():
        if q in params:
            raise ValueError(f"nuisance {q!r} is a fitted parameter (a parameter is fitted or budgeted, not both)")
        try:
            kind_q, mat_q, _ = _resolve_param(cfg, q)
        except ValueError as e:
            raise ValueError(f"nuisance {q!r}: {e}") from None
        if kind_q == "thickness":
            check_thickness_name(cfg, mat_q, q)
        try:
            ok = np.isfinite(float(sig)) and float(sig) > 0.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"nuisance {q!r}: the relative sigma must be positive and finite (got {sig!r})")
    check_capacity_names(params + tuple(nuisance))
    if nuisance:
        refuse_aniso(cfg, "heatflow_amd.fit with the conductivity of an anisotropic material as a nuisance", set(nuisance), DIRECTIONAL_HINT)
    thick = [(j, classify_param(p)[1]) for j, p in enumerate(params) if classify_param(p)[0] == "thickness"]
    for j, mat in thick:
        check_thickness_name(cfg, mat, params[j])
    exp = load_experiment(exp_csv)
    ic = float(cfg["heating"]["ic_temp"])
    stack = build_stack(cfg)
    own = session is None
    if own:
        if mesh is None:
            if rebuild_mesh is None:
                rebuild_mesh = not all(os.path.isfile(os.path.join(mesh_folder, f)) for f in ("mesh.msh", "mesh_cfg.yaml"))
            mesh = prepare_mesh(cfg, mesh_folder, rebuild_mesh, stack)
        coords, tris, tags, tag_map = mesh
        if not thick:
            session = SimulationSession(coords, tris, tags, tag_map, device_id=device_id, backend=backend, rtol=rtol)
    watchers = get_watcher_points(cfg)
    runs = tangent_runs = 0
    # thickness parameters: the triangles of the mesh of ``cfg`` stay and its nodes move,
    # z = z0 + sum_l V_l(z0) (theta_l - theta_l0), so the objective is smooth in theta and the tangent its exact derivative; every
    # new set of thicknesses gets a session of its own on the moved nodes (one resident at a time)
    moved = {"key": None, "session": None}
    if thick:
        if own:
            base, kw = (np.asarray(coords, dtype=np.float64), tris, tags, tag_map), dict(device_id=device_id, backend=backend, rtol=rtol)
        else:
            base = (session.coords, session.tris, session.tags, session.material_tags)
            kw = dict(device_id=session.device_id, backend=session.backend, rtol=session.rtol, max_it=session.max_it,
                      assembly_mode=session.assembly_mode, precond=session.precond)
        vel = {j: thickness_velocity(cfg, mat, base[0][:, 0]) for j, mat in thick}
        theta0 = {j: get_param(cfg, params[j]) for j, _ in thick}
        # the watcher nodes: those of the mesh of ``cfg``, followed as they move.  They are the nodes nearest to the moved
        # configuration's watcher points on the moved mesh, except that a tie (a coupler one element thick has its mid-plane
        # half-way between two nodes) is not decided anew by the rounding of every trial
        from .driver import _parse_watchers
        from .solver import nearest_nodes

        w_names, w_pts = _parse_watchers(watchers)
        w_nodes = nearest_nodes(base[0], w_pts)

    def session_for(theta):
        if not thick:
            return session
        key = tuple(float(theta[j]) for j, _ in thick)
        if moved["key"] != key:
            if moved["session"] is not None:
                moved["session"].close()
                moved["session"] = None
            c = np.array(base[0], dtype=np.float64)
            for j, _ in thick:
                c[:, 0] += vel[j] * (float(theta[j]) - theta0[j])
            moved["session"] = SimulationSession(c, base[1], base[2], base[3], **kw)
            moved["key"] = key
        return moved["session"]

    def run(theta, tangents):
        nonlocal runs, tangent_runs
        c = set_params(cfg, params, theta)
        s = session_for(theta)
        w = {nm: tuple(s.coords[i]) for nm, i in zip(w_names, w_nodes)} if thick else watchers
        res = s.run(c, build_stack(c), w, tangents=(params if tangents is True else tuple(tangents)) if tangents else None)
        if tangents:      # a table's scale: the run differentiates by a multiplier of the table as it stands, theta times the configuration's
            for j, p in enumerate(params):
                if p.endswith("_table.scale") and p in res["tangents"]:
                    res["tangents"][p] = {nm: d / float(theta[j]) for nm, d in res["tangents"][p].items()}
        runs += 1
        tangent_runs += bool(tangents)
        return res

    def resid_only(res):
        t_exp, y_exp, t_sim, y_sim = oside_curves(exp, ic, res["times"], res["watchers"]["pside"], res["watchers"]["oside"])
        return y_exp - np.interp(t_exp, t_sim, y_sim)

    try:
        theta = np.array([get_param(cfg, p) for p in params] if x0 is None else x0, dtype=np.float64)
        res = run(theta, True)
        r, J = residual_and_jacobian(res, params, exp, ic)
        cost = float(r @ r)
        lam = 1e-6
        history = [{"values": theta.tolist(), "rmse": float(np.sqrt(cost / len(r))), "lambda": lam}]
        it = 0
        converged = False
        while it < max_iter and not converged:
            it += 1
            Jl = J * theta                                   # d r / d log(theta)
            A, g = Jl.T @ Jl, Jl.T @ r
            while True:
                step = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
                pred = -(2.0 * g @ step + step @ A @ step)   # decrease of r.r the linearised model predicts
                if np.max(np.abs(step)) < xtol or pred <= ftol * cost:
                    converged = True                         # at the minimum to the model's resolution: no trial run
                    break
                trial = theta * np.exp(step)
                r_t = resid_only(run(trial, False))          # trial: the primal alone
                cost_t = float(r_t @ r_t)
                if cost_t <= cost:
                    theta, cost = trial, cost_t
                    lam = max(lam / 3.0, 1e-12)
                    res = run(theta, True)                   # accepted: the Jacobian there
                    r, J = residual_and_jacobian(res, params, exp, ic)
                    break
                lam *= 4.0
                if lam > 1e12:                               # no decrease along any damped step: a stationary point
                    converged = True
                    break
            history.append({"values": theta.tolist(), "rmse": float(np.sqrt(cost / len(r))), "lambda": lam})
            if verbose:
                print(f"fit iteration {it}: {dict(zip(params, theta))} rmse {np.sqrt(cost / len(r)):.6e}")
        m, p = len(r), len(params)
        s2 = cost / max(m - p, 1)
        try:
            stderr = np.sqrt(np.diag(s2 * np.linalg.inv(J.T @ J)))
        except np.linalg.LinAlgError:
            stderr = np.full(p, np.nan)
        budget = {}
        if nuisance:      # one tangent run at the fitted values with the columns params + nuisance
            names = params + tuple(nuisance)
            _, Jall = residual_and_jacobian(run(theta, names), names, exp, ic)
            Jp = Jall[:, :p]
            c_fit = set_params(cfg, params, theta)
            pinv = np.linalg.solve(Jp.T @ Jp, Jp.T)
            systematic = {}
            for k, (q, sig) in enumerate(nuisance.items()):
                shift = -(pinv @ Jall[:, p + k]) * (float(sig) * get_param(c_fit, q))
                systematic[q] = {nm: float(v) for nm, v in zip(params, shift)}
            budget = {"systematic": systematic,
                      "systematic_total": {nm: float(np.sqrt(sum(systematic[q][nm] ** 2 for q in systematic))) for nm in params}}
    finally:
        if own and session is not None:
            session.close()
        if moved["session"] is not None:
            moved["session"].close()
    return {"params": list(params), "values": theta.tolist(), "rmse": float(np.sqrt(cost / len(r))), "converged": bool(converged),
            "iterations": it, "history": history, "stderr": stderr.tolist(), "runs": runs, "tangent_runs": tangent_runs,
            "seconds": time.time() - t0, "tangent_iters_mean": float(np.mean(res["tangent_iters"])),
            "pcg_iters_mean": float(np.mean(res["iters"])), "scheme": scheme, "deformed_mesh": bool(thick), **budget}


def main(argv=None, backend=None):
    """The command line; ``backend`` (tests): a stand-in for the HIP backend."""
    import yaml

    ap = argparse.ArgumentParser(description="Fit conductivities (and fwhm) to the experimental o-side curve with tangent runs")
    ap.add_argument("--config", required=True)
    ap.add_argument("--params", nargs="+", default=["p_sample"], help="material names, <material>.k_r, <material>.k_z, <material>.k, <material>.thickness, <material>.rho_c, <material>.cv, <material>.rho, fwhm, and under heating.source.tangents: true source.fwhm, source.depth, source.pulse.t0, source.pulse.fwhm")
    ap.add_argument("--exp-csv", default=DEFAULT_EXP_CSV)
    ap.add_argument("--mesh-folder", default=None,
                    help="mesh.msh + mesh_cfg.yaml to use; built there when absent (default: <output-dir>/mesh)")
    ap.add_argument("--rebuild-mesh", action="store_true", help="build the mesh even if the folder holds one")
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--x0", nargs="+", type=float, default=None)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--scheme", choices=("backward_euler", "bdf2"), default=None,
                    help="time scheme (default: the configuration's timing.scheme, else backward_euler)")
    ap.add_argument("--nuisance", nargs="+", default=None, metavar="NAME=REL",
                    help="systematic-error budget: parameters that are assumed, not fitted, with their relative one-sigma "
                         "uncertainty, e.g. p_ins.rho_c=0.15 p_sample.thickness=0.05 fwhm=0.1")
    a = ap.parse_args(argv)
    nuisance = {}
    for item in a.nuisance or ():
        name, sep, rel = item.partition("=")
        try:
            nuisance[name] = float(rel)
        except ValueError:
            sep = ""
        if not sep or not name:
            ap.error(f"--nuisance {item!r}: NAME=REL expected")
    with open(a.config) as f:
        cfg = yaml.safe_load(f)
    if a.scheme is not None:
        cfg.setdefault("timing", {})["scheme"] = a.scheme
    os.makedirs(a.output_dir, exist_ok=True)
    mesh_folder = a.mesh_folder or os.path.join(a.output_dir, "mesh")
    out = fit_parameters(cfg, mesh_folder, a.params, a.exp_csv, a.x0, a.max_iter, device_id=a.device, backend=backend,
                         rebuild_mesh=True if a.rebuild_mesh else None, verbose=True, **({"nuisance": nuisance} if nuisance else {}))
    out["config"] = a.config
    with open(os.path.join(a.output_dir, "fit_summary.json"), "w") as f:
        json.dump(out, f, indent=2)
    from .driver import _dump_yaml, _with_scheme

    with open(os.path.join(a.output_dir, "used_config.yaml"), "w") as f:     # the configuration at the fitted values
        _dump_yaml(_with_scheme(set_params(cfg, out["params"], out["values"])), f)
    print(json.dumps({k: out[k] for k in ("params", "values", "stderr", "rmse", "converged", "iterations", "runs", "seconds", "scheme",
                                          "systematic", "systematic_total") if k in out}))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
