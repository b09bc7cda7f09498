"""Anisotropic conductivities of a configuration (hf_set_anisotropy).

A material keeps its ``k`` and may add ``k_aniso: {r: m_r, z: m_z}``: it then conducts with k_r = m_r k along the radius and
k_z = m_z k along the cell axis.  Either key may be absent and is then 1; both must be positive and finite.  Multipliers, not two
absolute values, so that everything that scales a material's ``k`` (kappa sweeps, ``--k-range``, the affine batch) keeps its
meaning: both directions scale and the ratio stays.

Combined with the temperature-dependent keys (k_table, k_power, cv_table, cv_einstein) in one configuration only under
``timing.aniso_tables: true`` (k_r = m_r kappa(T_e), k_z = m_z kappa(T_e), forward runs and the Picard steady
state; tangents, fits, sweeps and batches of such a configuration stay refused) - without the key the combination is refused,
the table kernels are isotropic - and never with the 1-D model.  Tangents and fits name the directional conductivities of a material as
``<material>.k_r`` and ``<material>.k_z`` (absolute, W/m/K) and its scalar as ``<material>.k`` (both directions, the ratio kept;
DESIGN.md 3.13); the bare name of an anisotropic material stays refused there.
"""
from __future__ import annotations

import math

from .kappa_t import CV_TABLE_KEYS, TABLE_KEYS, split_table_param, table_keys
from .source import SOURCE_PARAMS

KEY = "k_aniso"
SWITCH = "timing.aniso_tables"


def aniso_tables(cfg):
    """``timing.aniso_tables``: True opts in to ``k_aniso`` next to the kappa(T) / cv(T) keys (default off).
    ValueError naming the key for anything but true or false."""
    v = (cfg.get("timing") or {}).get("aniso_tables", False)
    if not isinstance(v, bool):
        raise ValueError(f"{SWITCH} must be true or false, got {v!r}")
    return v


def refuse_aniso_tables(cfg, where):
    """ValueError naming ``timing.aniso_tables`` and the keys if ``cfg`` sets the switch and carries both an anisotropic
    conductivity and a kappa(T) or cv(T) key: the switch covers forward runs and the Picard steady state, ``where`` is not among
    them.  Without the switch nothing is raised here: the caller's refusals of before follow, with the messages they had."""
    if not aniso_tables(cfg):
        return
    keys, tables = aniso_keys(cfg), table_keys(cfg, TABLE_KEYS + CV_TABLE_KEYS)
    if keys and tables:
        raise ValueError(f"{where}: {SWITCH} covers forward runs and the steady state only; anisotropic conductivities "
                         f"({', '.join(keys)}) together with temperature-dependent coefficients ({', '.join(tables)}) are not "
                         f"supported here")


def material_aniso(name, mat):
    """(m_r, m_z) of the material block ``mat`` (``mats.<name>``), or None when it has no ``k_aniso`` key.  ValueError naming
    the material for anything but ``{r: > 0, z: > 0}`` (either key optional)."""
    if not isinstance(mat, dict) or KEY not in mat:
        return None
    block = mat[KEY]
    if not isinstance(block, dict):
        raise ValueError(f"mats.{name}.{KEY}: a mapping with the keys r and / or z expected (got {block!r})")
    extra = sorted(str(k) for k in block if k not in ("r", "z"))
    if extra:
        raise ValueError(f"mats.{name}.{KEY}: unknown key(s) {', '.join(extra)} (r and z are the multipliers of k along r and z)")
    out = []
    for key in ("r", "z"):
        try:
            v = float(block.get(key, 1.0))
        except (TypeError, ValueError):
            raise ValueError(f"mats.{name}.{KEY}.{key}: not a number ({block.get(key)!r})") from None
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError(f"mats.{name}.{KEY}.{key} must be positive and finite (got {v!r})")
        out.append(v)
    return out[0], out[1]


PARAM_KINDS = {"k": "k", "k_r": "r", "k_z": "z"}     # suffix of a tangent / fit parameter -> column kind of run_tangent
THICKNESS = "thickness"                              # suffix of a layer-thickness parameter -> kind "t" (a shape column)
# suffixes of a heat-capacity parameter -> kind (a capacity column of run_tangent carries rho_c = rho * cv): the
# tangent in cv is rho times that column, the tangent in rho is cv times it
CAPACITY_KINDS = {"rho_c": "c", "cv": "cv", "rho": "rho"}


def split_param(name):
    """("<material>", "k" | "r" | "z") of a parameter spelt ``<material>.k``, ``<material>.k_r`` or ``<material>.k_z``,
    ("<material>", "t") of ``<material>.thickness``, ("<material>", "c" | "cv" | "rho") of ``<material>.rho_c``, ``<material>.cv``
    or ``<material>.rho``; (name, None) for a name without a dot.  ValueError naming the parameter for any other suffix."""
    if "." not in name:
        return name, None
    mat, suffix = name.rsplit(".", 1)
    if suffix == THICKNESS:
        return mat, "t"
    if suffix in CAPACITY_KINDS:
        return mat, CAPACITY_KINDS[suffix]
    if suffix not in PARAM_KINDS:
        raise ValueError(f"parameter {name!r}: unknown suffix {suffix!r} (<material>.k, <material>.k_r, <material>.k_z or "
                         f"<material>.thickness)")
    return mat, PARAM_KINDS[suffix]


def classify_param(name, tables=True):
    """(kind, material) of a tangent / fit parameter by its spelling alone - the one grammar of tangents=, monitor_sigma=,
    fit.get_param and fit.set_params: ("fwhm", None); ("source", None) for every "source.*" name (source.check_source_param tells
    the source's own from a misspelt one); ("table", <m>) for a name of kappa_t.TABLE_PARAM_SUFFIXES (``tables`` False: such a
    name is an unknown suffix, as in a run without tables); else the suffix as the kind, "k" | "k_r" | "k_z" | "thickness" | "rho_c"
    | "cv" | "rho", "k" also for the bare "<m>".  :func:`split_param`'s ValueError for any other suffix.  Whether the material
    exists, reads its thickness or carries the table is the caller's to check, against what it holds."""
    if name == "fwhm":
        return "fwhm", None
    if name in SOURCE_PARAMS or name.startswith("source."):
        return "source", None
    if tables and split_table_param(name) is not None:
        return "table", split_table_param(name)[0]
    mat, _ = split_param(name)
    return (name.rsplit(".", 1)[1] if "." in name else "k"), mat


def aniso_keys(cfg, names=None):
    """['mats.<name>.k_aniso', ...] of the materials of ``cfg`` (of ``names`` only, when given) that carry the key."""
    return [f"mats.{name}.{KEY}" for name, mat in sorted((cfg.get("mats") or {}).items())
            if isinstance(mat, dict) and KEY in mat and (names is None or name in names)]


def check_config(cfg):
    """Every ``k_aniso`` block of ``cfg`` parsed (ValueError for a bad one), and ValueError naming the keys if the configuration
    also carries a kappa(T) or cv(T) key without ``timing.aniso_tables: true``.  Returns {material name: (m_r, m_z)}."""
    both = aniso_tables(cfg)
    out = {}
    for name, mat in sorted((cfg.get("mats") or {}).items()):
        m = material_aniso(name, mat)
        if m is not None:
            out[name] = m
    if out and not both:
        tables = table_keys(cfg, TABLE_KEYS + CV_TABLE_KEYS)
        if tables:
            raise ValueError(f"anisotropic conductivities ({', '.join(aniso_keys(cfg))}) are not supported together with "
                             f"temperature-dependent coefficients ({', '.join(tables)}): the table kernels are isotropic")
    return out


DIRECTIONAL_HINT = ("; name the directional conductivities <material>.k_r / <material>.k_z, or the scalar <material>.k of both "
                    "directions, instead")


def refuse_aniso(cfg, where, names=None, hint=""):
    """ValueError naming the keys if ``cfg`` (its materials ``names`` only, when given) asks for an anisotropic conductivity:
    ``where`` does not support it.  ``hint`` is appended to the message."""
    keys = aniso_keys(cfg, names)
    if keys:
        raise ValueError(f"{where} does not support anisotropic conductivities ({', '.join(keys)}){hint}")


def capacity_scale(mat, kind):
    """The factor that turns the tangent in rho_c = rho * cv of the material block ``mat`` into the tangent in the parameter of
    ``kind``: 1 for "c" (rho_c itself), rho for "cv", cv for "rho"."""
    return 1.0 if kind == "c" else float(mat["rho"]) if kind == "cv" else float(mat["cv"])


def check_capacity_names(names):
    """ValueError naming both if two of ``<material>.rho_c``, ``<material>.cv`` and ``<material>.rho`` of one material are among
    ``names``: they move the same rho * cv, so they are not independent."""
    seen = {}
    for name in names:
        if "." not in name:
            continue
        mat, suffix = name.rsplit(".", 1)
        if suffix in CAPACITY_KINDS:
            if mat in seen:
                raise ValueError(f"parameters {seen[mat]!r} and {name!r} are not independent: both move rho * cv of {mat!r}")
            seen[mat] = name
