"""Temperature-dependent conductivities: tables from configuration keys and the refusals of the paths that
do not support them.

A material of ``cfg["mats"]`` may carry, besides its constant ``k``:
  ``k_table: {T_min, T_max, k: [...]}``                 values on a uniform grid from T_min to T_max (2..256 knots)
  ``k_power: {T_ref, exponent, T_min, T_max[, knots]}``  k (T_ref / T)^exponent tabulated on [T_min, T_max] (default 256 knots),
                                                        with the material's ``k`` as the value at T_ref
and, besides its constant ``cv``:
  ``cv_table: {T_min, T_max, cv: [...]}``               values of cv on a uniform grid; the table handed down is rho * cv
  ``cv_einstein: {theta, T_ref, T_min, T_max[, knots]}`` rho cv E(theta / T) / E(theta / T_ref), E(x) = x^2 e^x / (e^x - 1)^2 (an
                                                        Einstein solid), with the material's ``cv`` as the value at T_ref
and a latent heat (needs ``timing.capacity_form: enthalpy``):
  ``latent: {T_melt, heat, width[, T_min, T_max, knots]}`` a hat of base ``width`` centred at T_melt added to the material's rho * cv
                                                        table, carrying rho * heat (heat in J/kg); alone on its own grid, next
                                                        to cv_table / cv_einstein on theirs
The table is what the library evaluates: piecewise linear, clamped to the end values outside [T_min, T_max].
``timing.picard_sweeps`` (default 1) sets the Picard sweeps per step.  ``timing.capacity_form: lagged | enthalpy`` (absent:
lagged) chooses the form of the capacity; under the enthalpy form ``picard_sweeps`` is the sweep cap (1..64),
``timing.picard_tol`` (K, optional, >= 0) the stop tolerance and ``timing.picard_relax`` (in (0, 1], default 1) the relaxation.
"""
from __future__ import annotations

import numpy as np

MAX_KNOTS = 256
MAX_PICARD = 8
MAX_SWEEPS = 64          # the sweep cap of the enthalpy form
TABLE_KEYS = ("k_table", "k_power")
CV_TABLE_KEYS = ("cv_table", "cv_einstein", "latent")
FORM_KEY = "timing.capacity_form"
SWEEP_SWITCH = "timing.sweep_tables"


def power_law_table(k_ref, T_ref, exponent, T_min, T_max, knots=MAX_KNOTS):
    """(T0, dT, values) of k_ref (T_ref / T)^exponent at ``knots`` uniform points of [T_min, T_max]."""
    knots = int(knots)
    if not 2 <= knots <= MAX_KNOTS:
        raise ValueError(f"k_power: knots must be 2..{MAX_KNOTS} (got {knots})")
    T_min, T_max, T_ref = float(T_min), float(T_max), float(T_ref)
    if not (0.0 < T_min < T_max) or not T_ref > 0.0 or not float(k_ref) > 0.0:
        raise ValueError("k_power: need 0 < T_min < T_max, T_ref > 0 and k > 0")
    dT = (T_max - T_min) / (knots - 1)
    T = T_min + dT * np.arange(knots)
    return T_min, dT, float(k_ref) * (T_ref / T) ** float(exponent)


def uniform_table(T_min, T_max, values):
    """(T0, dT, values) of values given on a uniform grid from T_min to T_max."""
    v = np.asarray(values, dtype=np.float64).ravel()
    if not 2 <= v.size <= MAX_KNOTS:
        raise ValueError(f"k_table: 2..{MAX_KNOTS} values needed (got {v.size})")
    if not float(T_max) > float(T_min) or not np.all(v > 0.0) or not np.all(np.isfinite(v)):
        raise ValueError("k_table: need T_max > T_min and positive values")
    return float(T_min), (float(T_max) - float(T_min)) / (v.size - 1), v


def material_table(name, mat):
    """The (T0, dT, values) table of one material entry of cfg["mats"], or None without a table key."""
    if "k_table" in mat and "k_power" in mat:
        raise ValueError(f"mats.{name}: k_table and k_power are exclusive")
    if "k_table" in mat:
        t = mat["k_table"]
        return uniform_table(t["T_min"], t["T_max"], t["k"])
    if "k_power" in mat:
        p = mat["k_power"]
        return power_law_table(mat["k"], p["T_ref"], p["exponent"], p["T_min"], p["T_max"], p.get("knots", MAX_KNOTS))
    return None


def einstein_function(x):
    """E(x) = x^2 e^x / (e^x - 1)^2: the heat capacity of an Einstein solid over its Dulong-Petit limit, x = theta / T."""
    x = np.asarray(x, dtype=np.float64)
    ex = np.exp(x)
    return x * x * ex / (ex - 1.0) ** 2


def einstein_table(rho_cv_ref, theta, T_ref, T_min, T_max, knots=MAX_KNOTS):
    """(T0, dT, values) of rho_cv_ref E(theta / T) / E(theta / T_ref) at ``knots`` uniform points of [T_min, T_max]."""
    knots = int(knots)
    if not 2 <= knots <= MAX_KNOTS:
        raise ValueError(f"cv_einstein: knots must be 2..{MAX_KNOTS} (got {knots})")
    T_min, T_max, T_ref, theta = float(T_min), float(T_max), float(T_ref), float(theta)
    if not (0.0 < T_min < T_max) or not T_ref > 0.0 or not theta > 0.0 or not float(rho_cv_ref) > 0.0:
        raise ValueError("cv_einstein: need 0 < T_min < T_max, T_ref > 0, theta > 0 and rho cv > 0")
    dT = (T_max - T_min) / (knots - 1)
    T = T_min + dT * np.arange(knots)
    v = float(rho_cv_ref) * (einstein_function(theta / T) / float(einstein_function(theta / T_ref)))   # exactly rho cv at a knot T_ref
    if not np.all(v > 0.0) or not np.all(np.isfinite(v)):
        raise ValueError("cv_einstein: the table is not positive and finite on [T_min, T_max] (theta / T_min too large)")
    return T_min, dT, v


def latent_hat(name, mat, T0, dT, knots):
    """The values a ``latent`` block adds at the knots T0 + i dT: the hat of base ``width`` centred at ``T_melt``, sampled at the
    knots and rescaled so that the trapezoid integral of the added part is rho * heat exactly - the table's own integral, which is
    the H the enthalpy form conserves, then carries the configured latent heat.  ValueError for a hat with fewer than three knots
    inside its support (naming ``width`` and the grid spacing) or outside the grid."""
    b = mat["latent"]
    unknown = sorted(set(b) - {"T_melt", "heat", "width", "T_min", "T_max", "knots"})
    if unknown:
        raise ValueError(f"mats.{name}.latent: unknown key {unknown[0]!r} (T_melt, heat, width, T_min, T_max, knots)")
    for key in ("T_melt", "heat", "width"):
        if key not in b:
            raise ValueError(f"mats.{name}.latent: {key} is missing")
    T_melt, heat, width, rho = float(b["T_melt"]), float(b["heat"]), float(b["width"]), float(mat["rho"])
    if not (heat > 0.0 and width > 0.0 and rho > 0.0 and np.isfinite(heat) and np.isfinite(width) and np.isfinite(T_melt)):
        raise ValueError(f"mats.{name}.latent: need heat > 0 (J/kg), width > 0 (K), a finite T_melt and rho > 0")
    T = T0 + dT * np.arange(knots)
    hat = np.maximum(0.0, 1.0 - np.abs(T - T_melt) / (0.5 * width))
    inside = int(np.count_nonzero(hat > 0.0))
    if T_melt - 0.5 * width < T[0] or T_melt + 0.5 * width > T[-1]:
        raise ValueError(f"mats.{name}.latent: the hat {T_melt - 0.5 * width:g}..{T_melt + 0.5 * width:g} K leaves the table's grid "
                         f"{T[0]:g}..{T[-1]:g} K")
    if inside < 3:
        raise ValueError(f"mats.{name}.latent: width = {width:g} K holds {inside} knot(s) of a grid with spacing {dT:g} K (at least "
                         "three are needed inside the hat: widen it or refine the grid)")
    area = float(np.sum(0.5 * (hat[1:] + hat[:-1]) * dT))
    return hat * (rho * heat / area)


def material_cv_table(name, mat):
    """The (T0, dT, values of rho * cv) capacity table of one material entry of cfg["mats"], or None without a cv key.  A
    ``latent`` block adds its hat (latent_hat): alone on its own grid (T_min, T_max, knots; the base is the constant rho * cv),
    next to cv_table / cv_einstein on theirs (then T_min / T_max / knots in the block are a ValueError)."""
    if "latent" in mat:
        base = _material_cv_base(name, mat)
        b = mat["latent"]
        if not isinstance(b, dict):
            raise ValueError(f"mats.{name}.latent: a block {{T_melt, heat, width, ...}} expected")
        if base is not None:
            own = [k for k in ("T_min", "T_max", "knots") if k in b]
            other = "cv_table" if "cv_table" in mat else "cv_einstein"
            if own:
                raise ValueError(f"mats.{name}.latent.{own[0]} together with mats.{name}.{other} is not supported (the hat is sampled "
                                 f"on the grid of {other})")
            T0, dT, v = base
        else:
            for key in ("T_min", "T_max"):
                if key not in b:
                    raise ValueError(f"mats.{name}.latent: {key} is missing (the block's own grid; or give cv_table / cv_einstein)")
            knots = int(b.get("knots", MAX_KNOTS))
            if not 3 <= knots <= MAX_KNOTS:
                raise ValueError(f"mats.{name}.latent: knots must be 3..{MAX_KNOTS} (got {knots})")
            T0, T1, rc = float(b["T_min"]), float(b["T_max"]), float(mat["rho"]) * float(mat["cv"])
            if not T1 > T0 or not rc > 0.0:
                raise ValueError(f"mats.{name}.latent: need T_max > T_min and rho cv > 0")
            dT, v = (T1 - T0) / (knots - 1), np.full(knots, rc)
        return T0, dT, np.asarray(v, dtype=np.float64) + latent_hat(name, mat, T0, dT, len(v))
    return _material_cv_base(name, mat)


def _material_cv_base(name, mat):
    """material_cv_table without the ``latent`` block."""
    if "cv_table" in mat and "cv_einstein" in mat:
        raise ValueError(f"mats.{name}: cv_table and cv_einstein are exclusive")
    if "cv_table" in mat:
        t = mat["cv_table"]
        v = np.asarray(t["cv"], dtype=np.float64).ravel()
        if not 2 <= v.size <= MAX_KNOTS:
            raise ValueError(f"cv_table: 2..{MAX_KNOTS} values needed (got {v.size})")
        rho = float(mat["rho"])
        if not float(t["T_max"]) > float(t["T_min"]) or not rho > 0.0 or not np.all(v > 0.0) or not np.all(np.isfinite(v)):
            raise ValueError("cv_table: need T_max > T_min, rho > 0 and positive values")
        return float(t["T_min"]), (float(t["T_max"]) - float(t["T_min"])) / (v.size - 1), rho * v
    if "cv_einstein" in mat:
        p = mat["cv_einstein"]
        return einstein_table(float(mat["rho"]) * float(mat["cv"]), p["theta"], p["T_ref"], p["T_min"], p["T_max"],
                              p.get("knots", MAX_KNOTS))
    return None


def picard_sweeps(cfg):
    """``timing.picard_sweeps`` (default 1), checked against 1..8; under ``timing.capacity_form: enthalpy`` the sweep cap, 1..64."""
    raw = (cfg.get("timing") or {}).get("picard_sweeps", 1)
    top = MAX_SWEEPS if capacity_form(cfg) == "enthalpy" else MAX_PICARD
    p = int(raw or 1) if top == MAX_PICARD or raw is None else int(raw)      # (the lagged form reads 0 as absent, as it did)
    if not 1 <= p <= top:
        raise ValueError(f"timing.picard_sweeps must be 1..{top} (got {p})"
                         + (f" under {FORM_KEY}: enthalpy" if top == MAX_SWEEPS else ""))
    return p


def capacity_form(cfg):
    """``timing.capacity_form``: "lagged" (also when absent) or "enthalpy"; ValueError naming the key for anything else."""
    v = (cfg.get("timing") or {}).get("capacity_form", "lagged")
    if v is None:
        v = "lagged"
    if v not in ("lagged", "enthalpy"):
        raise ValueError(f"{FORM_KEY} must be lagged or enthalpy, got {v!r}")
    return v


def picard_control(cfg):
    """(tol or None, relax) of ``timing.picard_tol`` (K, >= 0) and ``timing.picard_relax`` (in (0, 1], default 1): ValueError
    naming the key for a value outside, and naming both keys for either one without ``timing.capacity_form: enthalpy``."""
    timing = cfg.get("timing") or {}
    tol, relax = timing.get("picard_tol"), timing.get("picard_relax")
    if capacity_form(cfg) != "enthalpy":
        for key, v in (("picard_tol", tol), ("picard_relax", relax)):
            if v is not None:
                raise ValueError(f"timing.{key} needs {FORM_KEY}: enthalpy (the lagged form takes a fixed number of sweeps)")
        return None, 1.0
    if tol is not None:
        try:
            tol = float(tol)
        except (TypeError, ValueError):
            raise ValueError(f"timing.picard_tol must be a tolerance >= 0 in K, got {tol!r}") from None
        if not (tol >= 0.0 and np.isfinite(tol)):
            raise ValueError(f"timing.picard_tol must be a tolerance >= 0 in K, got {tol!r}")
    try:
        relax = 1.0 if relax is None else float(relax)
    except (TypeError, ValueError):
        raise ValueError(f"timing.picard_relax must be in (0, 1], got {relax!r}") from None
    if not 0.0 < relax <= 1.0:
        raise ValueError(f"timing.picard_relax must be in (0, 1], got {relax!r}")
    return tol, relax


def latent_keys(cfg):
    return table_keys(cfg, ("latent",))


def check_capacity_form(cfg):
    """The combinations of the enthalpy form's keys a forward run refuses, each a ValueError naming both keys: ``latent`` without
    ``timing.capacity_form: enthalpy``; the enthalpy form without a capacity table, with ``timing.scheme: bdf2``, a ``k_aniso``,
    ``timing.sweep_tables`` or ``timing.table_tangents``.  Also checks the values of the form's own keys.  Returns the form."""
    form = capacity_form(cfg)
    lat = latent_keys(cfg)
    if form != "enthalpy" and lat:
        raise ValueError(f"{lat[0]} needs {FORM_KEY}: enthalpy (a step of the lagged form that jumps across the bump never sees it)")
    picard_control(cfg)
    picard_sweeps(cfg)
    if form != "enthalpy":
        return form
    timing = cfg.get("timing") or {}
    if not table_keys(cfg, CV_TABLE_KEYS):
        raise ValueError(f"{FORM_KEY}: enthalpy needs a capacity table (mats.<name>.cv_table, cv_einstein or latent)")
    if (timing.get("scheme") or "backward_euler") != "backward_euler":
        raise ValueError(f"{FORM_KEY}: enthalpy together with timing.scheme: {timing.get('scheme')} is not supported (backward "
                         "Euler only)")
    aniso = [f"mats.{name}.k_aniso" for name, mat in sorted((cfg.get("mats") or {}).items()) if isinstance(mat, dict) and "k_aniso" in mat]
    if aniso:
        raise ValueError(f"{FORM_KEY}: enthalpy together with {aniso[0]} is not supported (also with timing.aniso_tables: the "
                         "enthalpy kernel is isotropic)")
    if timing.get("sweep_tables"):
        raise ValueError(f"{FORM_KEY}: enthalpy together with {SWEEP_SWITCH} is not supported (the batch under tables takes the "
                         "lagged form)")
    if timing.get("table_tangents"):
        raise ValueError(f"{FORM_KEY}: enthalpy together with timing.table_tangents is not supported (tangent runs take the lagged "
                         "form)")
    return form


def refuse_enthalpy(cfg, where):
    """ValueError naming the key and ``where`` if ``cfg`` asks for the enthalpy form (or a ``latent`` block): ``where`` - tangents=,
    monitor_sigma=, heatflow_amd.fit, the sweeps, run_batch, the 1-D model - runs the lagged form only."""
    if capacity_form(cfg) == "enthalpy":
        raise ValueError(f"{where} together with {FORM_KEY}: enthalpy is not supported (it runs the lagged form only)")
    lat = latent_keys(cfg)
    if lat:
        raise ValueError(f"{where} together with {lat[0]} is not supported ({lat[0]} needs {FORM_KEY}: enthalpy, which {where} does "
                         "not run)")


def table_keys(cfg, keys=TABLE_KEYS + CV_TABLE_KEYS):
    """['mats.<name>.k_table', ...] of every material of ``cfg`` that carries a kappa(T) or cv(T) key (one of ``keys``)."""
    out = []
    for name, mat in sorted((cfg.get("mats") or {}).items()):
        for key in keys:
            if isinstance(mat, dict) and key in mat:
                out.append(f"mats.{name}.{key}")
    return out


def refuse_tables(cfg, where):
    """ValueError naming the key if ``cfg`` asks for kappa(T) or cv(T): ``where`` does not support it (yet)."""
    keys = table_keys(cfg, TABLE_KEYS)
    if keys:
        raise ValueError(f"{where} does not support temperature-dependent conductivities ({', '.join(keys)})")
    keys = table_keys(cfg, CV_TABLE_KEYS)
    if keys:
        raise ValueError(f"{where} does not support temperature-dependent heat capacities ({', '.join(keys)})")




def sweep_tables(cfg):
    """``timing.sweep_tables``: True opts in to kappa(T) / cv(T) keys in the sweeps and the batched loop (default
    off).  ValueError naming the key for anything but true or false."""
    v = (cfg.get("timing") or {}).get("sweep_tables", False)
    if not isinstance(v, bool):
        raise ValueError(f"{SWEEP_SWITCH} must be true or false, got {v!r}")
    return v


def refuse_tables_unless_swept(cfg, where):
    """:func:`refuse_tables` unless ``timing.sweep_tables`` is set: the three sweep entry points' check."""
    if not sweep_tables(cfg):
        refuse_tables(cfg, where)


def check_sweep_tables(cfg, where, swept=()):
    """What stays refused under ``timing.sweep_tables: true`` for a configuration with tables: ValueError naming both keys (or
    the argument) involved.  ``swept``: the materials whose ``k`` a kappa sweep varies."""
    if not sweep_tables(cfg) or not table_keys(cfg):
        return
    tables = ", ".join(table_keys(cfg))
    timing = cfg.get("timing") or {}
    if picard_sweeps(cfg) > 1:
        raise ValueError(f"{where}: timing.picard_sweeps = {picard_sweeps(cfg)} together with {SWEEP_SWITCH} is not supported "
                         "(the batch under tables takes one sweep per step, picard_sweeps: 1)")
    aniso = [f"mats.{name}.k_aniso" for name, mat in sorted((cfg.get("mats") or {}).items()) if isinstance(mat, dict) and "k_aniso" in mat]
    if aniso:
        extra = " (also with timing.aniso_tables)" if timing.get("aniso_tables") else ""
        raise ValueError(f"{where}: {', '.join(aniso)} together with {SWEEP_SWITCH} is not supported{extra}: the batch under tables "
                         f"({tables}) is isotropic")
    if isinstance(cfg.get("heating"), dict) and cfg["heating"].get("source") is not None:
        raise ValueError(f"{where}: heating.source together with {SWEEP_SWITCH} is not supported (also with heating.source.sweeps: "
                         f"true): the batch under tables ({tables}) has no source")
    if cfg.get("monitors") is not None:
        raise ValueError(f"{where}: monitors together with {SWEEP_SWITCH} is not supported (also with timing.sweep_monitors: true): "
                         f"the batch under tables ({tables}) keeps no records")
    if table_tangents(cfg):
        raise ValueError(f"{where}: timing.table_tangents together with {SWEEP_SWITCH} is not supported (batched columns have no "
                         "tangents)")
    for name in swept:
        mat = (cfg.get("mats") or {}).get(name)
        keys = [k for k in TABLE_KEYS if isinstance(mat, dict) and k in mat]
        if keys:
            raise ValueError(f"{where}: a k range over {name} together with mats.{name}.{keys[0]} is not supported under "
                             f"{SWEEP_SWITCH} (per-column tables: every point shares the tables)")


def table_derivative(mat, name):
    """(kind, values): the derivative of a material's table with respect to the parameter ``name``, at the table's own knots
    (DESIGN.md 3.20).  ``mat`` is the material's entry of cfg["mats"], ``kind`` "kappa" or "rhoc" (the keys of
    HeatProblem.run_tangent's ``tables=``).  The interpolation is linear in the knot values, so the derivative of the table is the
    table of the knots' derivatives.  Names (``<m>`` = the material):
      k_power      ``<m>`` / ``<m>.k``: table / k;   ``<m>.k_power.exponent``: table ln(T_ref / T_i)
      k_table      ``<m>.k_table.scale`` (a multiplier at 1): table
      cv_einstein  ``<m>.cv`` / ``<m>.rho`` / ``<m>.rho_c``: table / value;   ``<m>.cv_einstein.theta``: the analytic derivative
      cv_table     ``<m>.cv_table.scale``: table
    ValueError for a name the material's tables do not depend on this way."""
    m, _, suffix = str(name).partition(".")
    if suffix in ("", "k", "k_power.exponent", "k_table.scale"):
        tab = material_table(m, mat)
        if tab is None:
            raise ValueError(f"{name}: material {m} has no conductivity table")
        T0, dT, v = tab
        v = np.asarray(v, dtype=np.float64)
        if "k_table" in mat:
            if suffix != "k_table.scale":
                raise ValueError(f"{name}: a k_table material has no k to differentiate; its parameter is {m}.k_table.scale")
            return "kappa", v.copy()
        if suffix == "k_table.scale":
            raise ValueError(f"{name}: material {m} has a k_power table, not a k_table ({m}.k or {m}.k_power.exponent)")
        if suffix in ("", "k"):
            return "kappa", v / float(mat["k"])
        T = T0 + dT * np.arange(v.size)
        return "kappa", v * np.log(float(mat["k_power"]["T_ref"]) / T)
    if suffix in ("cv", "rho", "rho_c", "cv_einstein.theta", "cv_table.scale"):
        tab = material_cv_table(m, mat)
        if tab is None:
            raise ValueError(f"{name}: material {m} has no capacity table")
        T0, dT, v = tab
        v = np.asarray(v, dtype=np.float64)
        if "cv_table" in mat:
            if suffix != "cv_table.scale":
                raise ValueError(f"{name}: a cv_table material is differentiated through {m}.cv_table.scale only")
            return "rhoc", v.copy()
        if suffix == "cv_table.scale":
            raise ValueError(f"{name}: material {m} has a cv_einstein table, not a cv_table")
        if suffix in ("cv", "rho"):
            return "rhoc", v / float(mat[suffix])
        if suffix == "rho_c":
            return "rhoc", v / (float(mat["rho"]) * float(mat["cv"]))
        p = mat["cv_einstein"]
        T = T0 + dT * np.arange(v.size)
        dlnE = lambda x: 2.0 / x - 1.0 / np.tanh(0.5 * x)      # d ln E / dx, E = einstein_function
        theta, T_ref = float(p["theta"]), float(p["T_ref"])
        return "rhoc", v * (dlnE(theta / T) / T - dlnE(theta / T_ref) / T_ref)
    raise ValueError(f"{name}: not a table parameter (.k, .k_power.exponent, .k_table.scale, .cv, .rho, .rho_c, "
                     ".cv_einstein.theta, .cv_table.scale)")


# -- tangent runs and fits under tables (timing.table_tangents) -------------------------------------------------
TABLE_PARAM_SUFFIXES = ("k_power.exponent", "k_table.scale", "cv_einstein.theta", "cv_table.scale")


def table_tangents(cfg):
    """``timing.table_tangents``: the opt-in for tangent runs, fits and budgets of a configuration with tables (default off)."""
    return bool((cfg.get("timing") or {}).get("table_tangents", False))


def split_table_param(name):
    """("<material>", suffix) of a name that ends in one of TABLE_PARAM_SUFFIXES, None for any other name."""
    for suffix in TABLE_PARAM_SUFFIXES:
        if str(name).endswith("." + suffix) and len(name) > len(suffix) + 1:
            return name[:-len(suffix) - 1], suffix
    return None


def _table_material(cfg, name, mat):
    mats = cfg.get("mats") or {}
    if mat not in mats or not isinstance(mats[mat], dict):
        raise ValueError(f"parameter {name!r}: no material {mat!r} in the configuration")
    return mats[mat]


def table_param(cfg, name):
    """(material, kind, values) if ``name`` is a parameter of a table of ``cfg`` - one of TABLE_PARAM_SUFFIXES, or a bare material
    name / ``.k`` of a material with a conductivity table, or ``.cv`` / ``.rho`` / ``.rho_c`` of one with a capacity table -, the
    derivative table from :func:`table_derivative`; None for a name that no table depends on.  ValueError naming the parameter for
    a table name on a material without that table."""
    split = split_table_param(name)
    if split is not None:
        mat = split[0]
        block = _table_material(cfg, name, mat)
        if split[1].split(".")[0] not in block:
            raise ValueError(f"parameter {name!r}: material {mat!r} has no {split[1].split('.')[0]} block")
    else:
        mat, _, suffix = str(name).partition(".")
        block = (cfg.get("mats") or {}).get(mat)
        if not isinstance(block, dict):
            return None
        if suffix in ("", "k"):
            if not any(k in block for k in TABLE_KEYS):
                return None
        elif suffix in ("cv", "rho", "rho_c"):
            if not any(k in block for k in CV_TABLE_KEYS):
                return None
        else:
            return None
    kind, values = table_derivative(block, name)
    return mat, kind, values


def get_table_param(cfg, name):
    """The value of a name of TABLE_PARAM_SUFFIXES: the exponent, theta, or 1 for a scale (a multiplier of the table as it stands)."""
    mat, suffix = split_table_param(name)
    block = _table_material(cfg, name, mat)
    key, field = suffix.split(".")
    if key not in block:
        raise ValueError(f"parameter {name!r}: material {mat!r} has no {key} block")
    return 1.0 if field == "scale" else float(block[key][field])


def set_table_param(cfg, name, value):
    """Write a name of TABLE_PARAM_SUFFIXES into ``cfg`` (in place): the exponent or theta as given, a scale as the scaled list."""
    mat, suffix = split_table_param(name)
    block = _table_material(cfg, name, mat)
    key, field = suffix.split(".")
    if key not in block:
        raise ValueError(f"parameter {name!r}: material {mat!r} has no {key} block")
    if field == "scale":
        lst = "k" if key == "k_table" else "cv"
        block[key][lst] = [float(value) * float(v) for v in block[key][lst]]
    else:
        block[key][field] = float(value)


def check_table_tangents(cfg, where, names=()):
    """The refusals that stay under ``timing.table_tangents: true``: ValueError naming the argument for more than one Picard sweep, a
    volumetric source and a layer thickness among ``names``."""
    if picard_sweeps(cfg) > 1:
        raise ValueError(f"{where}: timing.picard_sweeps = {picard_sweeps(cfg)} (timing.table_tangents covers the lagged scheme, "
                         "picard_sweeps: 1)")
    if isinstance(cfg.get("heating"), dict) and cfg["heating"].get("source") is not None:
        raise ValueError(f"{where}: heating.source together with timing.table_tangents is not supported")
    for p in names:
        if str(p).endswith(".thickness"):
            raise ValueError(f"{where}: parameter {p!r}: a layer thickness together with timing.table_tangents is not supported")
        if str(p).startswith("source."):
            raise ValueError(f"{where}: parameter {p!r}: a source parameter together with timing.table_tangents is not supported")
