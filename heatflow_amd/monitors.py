"""Region monitors: the ``monitors`` block of a configuration and the combination of per-tag records.

    monitors:
      sample:  {material: p_sample, above: 2000.0}
      coupler: {material: [p_coupler, o_coupler]}

A region is a set of materials (cell tags).  After every step the GPU leaves one record row per monitored cell tag
(hf_set_monitors: T_max, node_max, T_min, node_min, I0 = int r dA, I1 = int u r dA, H = int over {u > above} of r dA); this module
combines the rows of a region's tags, in ascending tag order, into

    T_max, z_max, r_max     the peak nodal temperature of the region and where it sits
    T_min, z_min, r_min     the same for the lowest one
    volume                  2 pi sum I0
    T_mean                  sum I1 / sum I0, the volume average
    hot_volume, hot_fraction   2 pi sum H and sum H / sum I0 - only for a region with ``above``
    energy                  2 pi sum_t rho_c_t (I1_t - T_ref I0_t), the heat stored above T_ref = heating.ic_temp - left out when a
                            tag of the region carries a capacity table (the constant rho cv is then not the run's)

In tangent runs the GPU can also leave the derivatives of the sums along every tangent column (hf_set_monitor_tangents, DESIGN.md
3.18); :func:`combine_tangents` applies the chain rule per region and :func:`uncertainty` turns stated input uncertainties into
one-sigma bands.

It parses and validates the block and does the host arithmetic; it touches no GPU.
"""
from __future__ import annotations

import csv
import math

import numpy as np

KEY = "monitors"
REGION_KEYS = ("material", "above")
FIELDS = ("T_max", "z_max", "r_max", "T_min", "z_min", "r_min", "volume", "T_mean", "hot_volume", "hot_fraction", "energy")
F_TMAX, F_NMAX, F_TMIN, F_NMIN, F_I0, F_I1, F_H = range(7)      # columns of a record row (hf_get_monitors)


def monitors_block(cfg):
    """The raw ``monitors`` block of ``cfg``, or None when the key is absent (or null)."""
    return cfg.get(KEY)


def refuse_monitors(cfg, where):
    """ValueError naming the key if ``cfg`` asks for monitors: ``where`` does not support them."""
    if monitors_block(cfg) is not None:
        raise ValueError(f"{where} does not support region monitors ({KEY})")


def sweep_monitors(cfg):
    """``timing.sweep_monitors``: True opts in to the sweeps and run_batch with a ``monitors`` block (the block's own
    keys are region names, so the switch lives in ``timing``).  ValueError naming the key unless it is a bool."""
    v = (cfg.get("timing") or {}).get("sweep_monitors", False)
    if not isinstance(v, bool):
        raise ValueError(f"timing.sweep_monitors must be true or false, got {v!r}")
    return v


def refuse_monitors_sweeps(cfg, where):
    """:func:`refuse_monitors` unless ``timing.sweep_monitors`` opts in."""
    if not sweep_monitors(cfg):
        refuse_monitors(cfg, where)


def _above(region, value):
    if value is None:
        return None
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{KEY}.{region}.above: a number is expected, got {value!r}") from None
    if not math.isfinite(v):
        raise ValueError(f"{KEY}.{region}.above must be finite, got {value!r}")
    return v


def parse_monitors(cfg):
    """{region: {"materials": (names), "above": theta | None}} of ``cfg``'s ``monitors`` block in the block's order, or None when
    the key is absent.  ValueError naming the key, the region and the offender for an unknown key, an unknown material, a
    material listed twice, or an ``above`` that is not a finite number."""
    block = monitors_block(cfg)
    if block is None:
        return None
    if not isinstance(block, dict) or not block:
        raise ValueError(f"{KEY} must be a mapping of region names to {{material, above}}, got {block!r}")
    known = cfg.get("mats") or {}
    out = {}
    for region, spec in block.items():
        region = str(region)
        if "." in region or "," in region:
            raise ValueError(f"{KEY}: region name {region!r} must not contain '.' or ',' (it heads the columns of monitors.csv)")
        if not isinstance(spec, dict):
            raise ValueError(f"{KEY}.{region} must be a mapping {{material, above}}, got {spec!r}")
        for key in spec:
            if key not in REGION_KEYS:
                raise ValueError(f"{KEY}.{region}: unknown key {key!r} (expected one of {', '.join(REGION_KEYS)})")
        if "material" not in spec:
            raise ValueError(f"{KEY}.{region}.material is missing")
        mats = spec["material"]
        mats = [mats] if isinstance(mats, str) else list(mats or [])
        if not mats:
            raise ValueError(f"{KEY}.{region}.material names no material")
        for m in mats:
            if m not in known:
                raise ValueError(f"{KEY}.{region}.material: unknown material {m!r} (the configuration has {', '.join(sorted(known))})")
        if len(set(mats)) != len(mats):
            raise ValueError(f"{KEY}.{region}.material lists a material twice: {mats!r}")
        out[region] = {"materials": tuple(mats), "above": _above(region, spec.get("above"))}
    return out


def used_config(spec):
    """The block as it ran (used_config.yaml)."""
    return {region: {"material": list(r["materials"]), **({"above": r["above"]} if r["above"] is not None else {})}
            for region, r in spec.items()}


def problem_monitors(spec, material_tags):
    """The ``monitors=`` argument of HeatProblem: {region: {"tags": [cell tags], "above": theta | None}}."""
    return {region: {"tags": [int(material_tags[m]) for m in r["materials"]], "above": r["above"]} for region, r in spec.items()}


def check_regions(monitors):
    """{region: {"tags": [ascending ints], "above": float | None}} of HeatProblem's ``monitors=``, or None; ValueError naming
    ``monitors`` for an unknown key, a region without tags, a tag listed twice or a non-finite ``above`` (before any backend
    call)."""
    if not monitors:
        return None
    out = {}
    for region, spec in dict(monitors).items():
        spec = dict(spec)
        unknown = sorted(set(spec) - {"tags", "above"})
        if unknown:
            raise ValueError(f"monitors: region {region!r}: unknown key {unknown[0]!r} (tags, above)")
        tags = [int(t) for t in np.atleast_1d(spec.get("tags", []))]
        if not tags or len(set(tags)) != len(tags) or min(tags) < 0:
            raise ValueError(f"monitors: region {region!r}: tags must name at least one cell tag, each once (got {tags!r})")
        above = spec.get("above")
        if above is not None:
            above = float(above)
            if not math.isfinite(above):
                raise ValueError(f"monitors: region {region!r}: above must be finite (or None), got {spec.get('above')!r}")
        out[str(region)] = {"tags": sorted(tags), "above": above}
    return out


def tag_thresholds(regions):
    """{cell tag: theta | None} for hf_set_monitors: every tag of every region, with the region's ``above``.  A tag may sit in
    several regions, but a tag has one threshold: two different finite ``above`` values on it are a ValueError naming both
    regions."""
    out, owner = {}, {}
    for region, r in regions.items():
        for t in r["tags"]:
            if r["above"] is None:
                out.setdefault(t, None)
                continue
            if out.get(t) is not None and out[t] != r["above"]:
                raise ValueError(f"monitors: cell tag {t} is in region {owner[t]!r} with above = {out[t]!r} and in region "
                                 f"{region!r} with above = {r['above']!r} (a tag has one threshold)")
            out[t] = r["above"]
            owner[t] = region
    return out


def combine(records, regions, coords, rho_c=None, T_ref=None, tabled=()):
    """Per-tag records [K, tab_len, 7] (HeatflowHIP.get_monitors; one row [tab_len, 7] for a single record) -> {region: {field:
    array of K values}} (scalars for a single record).  ``coords`` (n, 2) [z, r] places the extremes; ``rho_c`` = {cell tag: rho cv}
    and ``T_ref`` give ``energy``, which is left out (key absent) without them or when a tag of the region is in ``tabled``
    (cell tags with a capacity table).  Every sum over the tags of a region runs in ascending tag order."""
    rec = np.asarray(records, dtype=np.float64)
    single = rec.ndim == 2
    if single:
        rec = rec[None]
    coords = np.asarray(coords, dtype=np.float64)
    tabled = {int(t) for t in tabled}
    two_pi = 2.0 * math.pi
    out = {}
    for region, r in regions.items():
        tags = sorted(int(t) for t in r["tags"])
        K = rec.shape[0]
        tmax = np.full(K, -np.inf)
        tmin = np.full(K, np.inf)
        nmax = np.zeros(K, dtype=np.int64)
        nmin = np.zeros(K, dtype=np.int64)
        s0, s1, sh = np.zeros(K), np.zeros(K), np.zeros(K)
        en = np.zeros(K)
        for t in tags:
            row = rec[:, t, :]
            up = row[:, F_TMAX] > tmax          # strictly: among equal peaks the lowest tag keeps it
            tmax = np.where(up, row[:, F_TMAX], tmax)
            nmax = np.where(up, row[:, F_NMAX].astype(np.int64), nmax)
            dn = row[:, F_TMIN] < tmin
            tmin = np.where(dn, row[:, F_TMIN], tmin)
            nmin = np.where(dn, row[:, F_NMIN].astype(np.int64), nmin)
            s0 = s0 + row[:, F_I0]
            s1 = s1 + row[:, F_I1]
            sh = sh + row[:, F_H]
            if rho_c is not None and T_ref is not None and t in rho_c:
                en = en + float(rho_c[t]) * (row[:, F_I1] - float(T_ref) * row[:, F_I0])
        with np.errstate(divide="ignore", invalid="ignore"):      # (a record of zeros, e.g. of a stand-in, gives nan means)
            f = {"T_max": tmax, "z_max": coords[nmax, 0], "r_max": coords[nmax, 1],
                 "T_min": tmin, "z_min": coords[nmin, 0], "r_min": coords[nmin, 1],
                 "volume": two_pi * s0, "T_mean": s1 / s0}
            if r["above"] is not None:
                f["hot_volume"] = two_pi * sh
                f["hot_fraction"] = sh / s0
        if rho_c is not None and T_ref is not None and all(t in rho_c for t in tags) and not (tabled & set(tags)):
            f["energy"] = two_pi * en
        out[region] = {k: (float(v[0]) if single else v) for k, v in f.items()}
    return out


TANGENT_FIELDS = ("T_max", "T_min", "volume", "T_mean", "hot_volume", "hot_fraction", "energy")
D_TMAX, D_TMIN, D_I0, D_I1, D_H = range(5)                        # fields of a derivative row (hf_get_monitor_tangents)


def combine_tangents(records, drecords, regions, rho_c=None, T_ref=None, tabled=(), capacity_columns=None, scale=None):
    """The chain rule of :func:`combine`: primal records [K, tab_len, 7] and the derivative records of the same
    states [K, tab_len, n_par, 5] (HeatflowHIP.get_monitor_tangents, fields dT_max, dT_min, dI0, dI1, dH) -> {region: {field:
    array (K, n_par)}} for T_max, T_min, volume, T_mean, hot_volume, hot_fraction and energy, the sums over a region's tags in
    ascending tag order:

        d volume = 2 pi sum dI0                       d T_mean = (sum dI1 - T_mean sum dI0) / sum I0
        d hot_volume = 2 pi sum dH                    d hot_fraction = (sum dH - hot_fraction sum dI0) / sum I0
        d T_max = dT_max of the tag that holds the region's peak (combine's tie rule: the lowest tag), d T_min likewise
        d energy = 2 pi sum_t rho_c_t (dI1_t - T_ref dI0_t), plus 2 pi (I1_t - T_ref I0_t) in the column that carries the
                   rho_c of tag t (``capacity_columns`` = {cell tag: column})

    ``scale`` (n_par values, default ones) multiplies whole columns, as the watcher tangents of ``.cv`` and ``.rho`` are scaled.
    ``hot_*`` and ``energy`` are left out wherever :func:`combine` leaves them out."""
    rec = np.asarray(records, dtype=np.float64)
    drec = np.asarray(drecords, dtype=np.float64)
    if rec.ndim == 2:
        rec = rec[None]
    if drec.ndim == 3:
        drec = drec[None]
    if rec.shape[0] != drec.shape[0] or rec.shape[1] != drec.shape[1]:
        raise ValueError(f"combine_tangents: records {rec.shape} and drecords {drec.shape} do not belong together")
    K, _, n_par, _ = drec.shape
    scale = np.ones(n_par) if scale is None else np.asarray(scale, dtype=np.float64).reshape(n_par)
    tabled = {int(t) for t in tabled}
    cap = {int(t): int(j) for t, j in (capacity_columns or {}).items()}
    two_pi = 2.0 * math.pi
    out = {}
    for region, r in regions.items():
        tags = sorted(int(t) for t in r["tags"])
        tmax, tmin = np.full(K, -np.inf), np.full(K, np.inf)
        dmax, dmin = np.zeros((K, n_par)), np.zeros((K, n_par))
        s0, s1, sh = np.zeros(K), np.zeros(K), np.zeros(K)
        d0, d1, dh, de = (np.zeros((K, n_par)) for _ in range(4))
        for t in tags:
            row, drow = rec[:, t, :], drec[:, t, :, :]
            up = row[:, F_TMAX] > tmax
            tmax = np.where(up, row[:, F_TMAX], tmax)
            dmax = np.where(up[:, None], drow[:, :, D_TMAX], dmax)
            dn = row[:, F_TMIN] < tmin
            tmin = np.where(dn, row[:, F_TMIN], tmin)
            dmin = np.where(dn[:, None], drow[:, :, D_TMIN], dmin)
            s0, s1, sh = s0 + row[:, F_I0], s1 + row[:, F_I1], sh + row[:, F_H]
            d0, d1, dh = d0 + drow[:, :, D_I0], d1 + drow[:, :, D_I1], dh + drow[:, :, D_H]
            if rho_c is not None and T_ref is not None and t in rho_c:
                de = de + float(rho_c[t]) * (drow[:, :, D_I1] - float(T_ref) * drow[:, :, D_I0])
                if t in cap and 0 <= cap[t] < n_par:
                    de[:, cap[t]] = de[:, cap[t]] + (row[:, F_I1] - float(T_ref) * row[:, F_I0])
        with np.errstate(divide="ignore", invalid="ignore"):
            mean, frac = (s1 / s0)[:, None], (sh / s0)[:, None]
            f = {"T_max": dmax, "T_min": dmin, "volume": two_pi * d0, "T_mean": (d1 - mean * d0) / s0[:, None]}
            if r["above"] is not None:
                f["hot_volume"] = two_pi * dh
                f["hot_fraction"] = (dh - frac * d0) / s0[:, None]
        if rho_c is not None and T_ref is not None and all(t in rho_c for t in tags) and not (tabled & set(tags)):
            f["energy"] = two_pi * de
        out[region] = {k: v * scale[None, :] for k, v in f.items()}
    return out


def csv_columns(history):
    """The columns of monitors.csv after ``time``: ``<region>.<field>`` in the regions' order, fields in FIELDS' order."""
    return [(region, field) for region, f in history.items() for field in FIELDS if field in f]


def write_monitors_csv(path, times, history):
    """``<out>/monitors.csv``: ``time, <region>.<field>, ...``, one row per step at the watcher CSV's times."""
    cols = csv_columns(history)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["time"] + [f"{region}.{field}" for region, field in cols])
        for k, t in enumerate(times):
            w.writerow([repr(float(t))] + [repr(float(history[region][field][k])) for region, field in cols])


def check_sigma(monitor_sigma):
    """{parameter: relative one-sigma} of the drivers' ``monitor_sigma=`` as floats; ValueError naming the argument for anything
    but a mapping of names to positive finite numbers."""
    if not isinstance(monitor_sigma, dict) or not monitor_sigma:
        raise ValueError(f"monitor_sigma must be a mapping {{parameter: relative one-sigma}}, got {monitor_sigma!r}")
    out = {}
    for name, v in monitor_sigma.items():
        try:
            f = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"monitor_sigma: {name}: a number is expected, got {v!r}") from None
        if not math.isfinite(f) or f <= 0.0:
            raise ValueError(f"monitor_sigma: {name}: the relative one-sigma must be positive and finite, got {v!r}")
        out[str(name)] = f
    return out


def uncertainty(derivatives, sigma_abs):
    """First-order one-sigma bands: ``derivatives`` = {param: {region: {field: d field / d param per step}}} and ``sigma_abs`` =
    {param: sigma_q theta_q} -> {region: {field: sqrt(sum_q (d field / d theta_q sigma_q theta_q)^2)}}, the parameters taken as
    independent."""
    out = {}
    for q, s in sigma_abs.items():
        for region, fields in derivatives[q].items():
            for field, d in fields.items():
                acc = out.setdefault(region, {})
                term = (np.asarray(d, dtype=np.float64) * float(s)) ** 2
                acc[field] = term if field not in acc else acc[field] + term
    return {region: {field: np.sqrt(v) for field, v in fields.items()} for region, fields in out.items()}


def write_uncertainty_csv(path, times, history, bands):
    """``<out>/monitor_uncertainty.csv``: ``time, <region>.<field>, <region>.<field>.sigma, ...`` for every field with a band, the
    regions in the monitors' order and the fields in FIELDS' order, one row per step."""
    cols = [(region, field) for region, field in csv_columns(history) if field in bands.get(region, {})]
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["time"] + [c for region, field in cols for c in (f"{region}.{field}", f"{region}.{field}.sigma")])
        for k, t in enumerate(times):
            w.writerow([repr(float(t))] + [repr(float(v)) for region, field in cols
                                           for v in (history[region][field][k], bands[region][field][k])])
