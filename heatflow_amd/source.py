"""Laser-power heating: the ``heating.source`` block of a configuration.

    heating:
      source:
        material: p_coupler        # a name or a list of names
        power: 0.5                 # absorbed peak power, W
        fwhm: 1.0e-5               # beam FWHM; defaults to heating.fwhm
        depth: 2.0e-8              # absorption length; absent = uniform through the layer
        face: outer                # outer | inner: which z face of the (first) material z0 is; default outer
        pulse: {t0: 1.0e-6, fwhm: 5.0e-7}     # Gaussian in time, peak 1; or {file: x.csv}
        keep_line: false           # true keeps the heated Dirichlet line as well
        tangents: true             # opt in to tangent runs, fits and monitor error bars under the source
        sweeps: true               # opt in to the sweeps and run_batch under the source

The source is q(z, r, t) = p(t) s(z, r) with s = exp(-4 ln2 r^2 / fwhm^2) exp(-|z - z0| / depth) inside the listed materials
(hf_set_source forms its load F1 on the GPU).  The absorbed power is P(t) = power * pulse(t); the amplitude handed to the time
loop is the peak power density p(t) = P(t) / (2 pi sum_i F1_i), because the hat functions sum to one: the configured power is the
discrete model's power exactly.  ``pulse`` is a Gaussian in time of peak 1, exp(-4 ln2 (t - t0)^2 / fwhm^2), or a CSV file with
the columns ``time`` and ``power`` (the pulse shape in units of ``power``; linear interpolation, 0 outside the file's times).

This module parses and validates the block and computes the amplitudes; it touches no GPU.
"""
from __future__ import annotations

import csv
import math
import os
from dataclasses import dataclass

import numpy as np

KEY = "heating.source"
SOURCE_KEYS = ("material", "power", "fwhm", "depth", "face", "pulse", "keep_line", "tangents", "sweeps")
# the source's own parameters in tangents=, monitor_sigma=, fits and --nuisance (under ``tangents: true``)
SOURCE_PARAMS = ("source.power", "source.fwhm", "source.depth", "source.pulse.t0", "source.pulse.fwhm")
PULSE_KEYS = ("t0", "fwhm", "file")
FACES = ("outer", "inner")


@dataclass(frozen=True)
class SourceSpec:
    """A validated ``heating.source`` block."""

    materials: tuple        # material names, the first one carries z0's face
    power: float            # absorbed peak power, W
    fwhm: float             # beam FWHM, m
    depth: float            # absorption length, m (inf: uniform through the layer)
    face: str               # "outer" | "inner"
    pulse: tuple            # ("gaussian", t0, fwhm) or ("file", path)
    keep_line: bool
    tangents: bool = False  # tangent runs, fits and monitor error bars are allowed under this source
    sweeps: bool = False    # run_parameter_sweep, run_kappa_sweep and run_batch are allowed under this source

    def z0(self, stack):
        """z of the absorbing face: the z face of the first material away from the sample mid-plane z = 0 (outer) or towards it
        (inner)."""
        box = stack.by_name(self.materials[0]).boundaries
        zmin, zmax = float(box[0]), float(box[1])
        outer_is_min = 0.5 * (zmin + zmax) < 0.0
        return zmin if outer_is_min == (self.face == "outer") else zmax

    def problem_source(self, stack, material_tags):
        """The ``source=`` argument of HeatProblem: cell tags, fwhm, z0, depth."""
        return {"tags": [int(material_tags[m]) for m in self.materials], "fwhm": self.fwhm, "z0": self.z0(stack),
                "depth": self.depth}

    def used_config(self):
        """The block as it ran, every default written out (used_config.yaml)."""
        out = {"material": list(self.materials), "power": self.power, "fwhm": self.fwhm, "face": self.face,
               "keep_line": self.keep_line}
        if math.isfinite(self.depth):
            out["depth"] = self.depth
        out["pulse"] = {"t0": self.pulse[1], "fwhm": self.pulse[2]} if self.pulse[0] == "gaussian" else {"file": self.pulse[1]}
        if self.tangents:
            out["tangents"] = True
        if self.sweeps:
            out["sweeps"] = True
        return out


def source_block(cfg):
    """The raw ``heating.source`` block of ``cfg``, or None when the key is absent (or null)."""
    return (cfg.get("heating") or {}).get("source")


def refuse_source(cfg, where):
    """ValueError naming the key if ``cfg`` asks for a volumetric source: ``where`` does not support it."""
    if source_block(cfg) is not None:
        raise ValueError(f"{where} does not support the volumetric source ({KEY})")


def source_permits_tangents(cfg):
    """True when ``cfg`` has a source that opts in to tangents (``heating.source.tangents: true``); a configuration without a
    source needs no permission and gives False."""
    block = source_block(cfg)
    return isinstance(block, dict) and block.get("tangents") is True


def refuse_source_tangents(cfg, where):
    """:func:`refuse_source` unless the source opts in to tangents."""
    if not source_permits_tangents(cfg):
        refuse_source(cfg, where)


def source_permits_sweeps(cfg):
    """True when ``cfg`` has a source that opts in to the sweeps (``heating.source.sweeps: true``); a configuration without a
    source needs no permission and gives False."""
    block = source_block(cfg)
    return isinstance(block, dict) and block.get("sweeps") is True


def refuse_source_sweeps(cfg, where):
    """:func:`refuse_source` unless the source opts in to the sweeps."""
    if not source_permits_sweeps(cfg):
        refuse_source(cfg, where)


def _positive(block, key, value):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{KEY}.{key}: a number is expected, got {value!r}") from None
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{KEY}.{key} must be positive and finite, got {value!r}")
    return v


def parse_source(cfg):
    """The :class:`SourceSpec` of ``cfg``'s ``heating.source`` block, or None when the key is absent.  ValueError naming the key
    or the material for an unknown key, an unknown material, a non-positive number, an unknown face, or both or neither form
    of ``pulse``."""
    block = source_block(cfg)
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError(f"{KEY} must be a mapping, got {block!r}")
    for key in block:
        if key not in SOURCE_KEYS:
            raise ValueError(f"{KEY}: unknown key {key!r} (expected one of {', '.join(SOURCE_KEYS)})")
    if "material" not in block:
        raise ValueError(f"{KEY}.material is missing")
    mats = block["material"]
    mats = [mats] if isinstance(mats, str) else list(mats or [])
    if not mats:
        raise ValueError(f"{KEY}.material names no material")
    known = cfg.get("mats") or {}
    for m in mats:
        if m not in known:
            raise ValueError(f"{KEY}.material: unknown material {m!r} (the configuration has {', '.join(sorted(known))})")
    if len(set(mats)) != len(mats):
        raise ValueError(f"{KEY}.material lists a material twice: {mats!r}")
    if "power" not in block:
        raise ValueError(f"{KEY}.power is missing")
    power = _positive(block, "power", block["power"])
    if "fwhm" in block:
        fwhm = _positive(block, "fwhm", block["fwhm"])
    elif "fwhm" in (cfg.get("heating") or {}):
        fwhm = _positive(block, "fwhm", cfg["heating"]["fwhm"])
    else:
        raise ValueError(f"{KEY}.fwhm is missing and there is no heating.fwhm to default to")
    depth = _positive(block, "depth", block["depth"]) if block.get("depth") is not None else math.inf
    face = block.get("face", "outer")
    if face not in FACES:
        raise ValueError(f"{KEY}.face must be one of {', '.join(FACES)}, got {face!r}")
    pulse = block.get("pulse")
    if not isinstance(pulse, dict):
        raise ValueError(f"{KEY}.pulse is missing: either {{t0, fwhm}} (a Gaussian in time) or {{file}} (a CSV)")
    for key in pulse:
        if key not in PULSE_KEYS:
            raise ValueError(f"{KEY}.pulse: unknown key {key!r} (expected t0 and fwhm, or file)")
    gaussian = "t0" in pulse or "fwhm" in pulse
    if gaussian == ("file" in pulse):
        raise ValueError(f"{KEY}.pulse needs exactly one form: either t0 and fwhm (a Gaussian in time) or file (a CSV)")
    if gaussian:
        if "t0" not in pulse or "fwhm" not in pulse:
            raise ValueError(f"{KEY}.pulse: a Gaussian pulse needs both t0 and fwhm")
        try:
            t0 = float(pulse["t0"])
        except (TypeError, ValueError):
            raise ValueError(f"{KEY}.pulse.t0: a number is expected, got {pulse['t0']!r}") from None
        if not math.isfinite(t0):
            raise ValueError(f"{KEY}.pulse.t0 must be finite, got {pulse['t0']!r}")
        spec = ("gaussian", t0, _positive(block, "pulse.fwhm", pulse["fwhm"]))
    else:
        spec = ("file", str(pulse["file"]))
    keep = block.get("keep_line", False)
    if not isinstance(keep, bool):
        raise ValueError(f"{KEY}.keep_line must be true or false, got {keep!r}")
    tangents = block.get("tangents", False)
    if not isinstance(tangents, bool):
        raise ValueError(f"{KEY}.tangents must be true or false, got {tangents!r}")
    sweeps = block.get("sweeps", False)
    if not isinstance(sweeps, bool):
        raise ValueError(f"{KEY}.sweeps must be true or false, got {sweeps!r}")
    return SourceSpec(tuple(mats), power, fwhm, depth, face, spec, keep, tangents, sweeps)


def read_pulse_csv(path):
    """(time, power) of a pulse file, sorted by time; ValueError when a column is missing or no row is numeric."""
    times, vals = [], []
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        cols = rd.fieldnames or []
        for c in ("time", "power"):
            if c not in cols:
                raise ValueError(f"{KEY}.pulse.file {path} must contain a '{c}' column")
        for row in rd:
            try:
                t, v = float(row["time"]), float(row["power"])
            except (TypeError, ValueError):
                continue
            if math.isnan(t) or math.isnan(v):
                continue
            times.append(t)
            vals.append(v)
    if not times:
        raise ValueError(f"{KEY}.pulse.file {path} holds no numeric rows")
    order = np.argsort(np.array(times), kind="stable")
    return np.array(times)[order], np.array(vals)[order]


def pulse_values(spec, times, resolve=None):
    """pulse(t) at ``times``: the Gaussian of peak 1, or the file's shape by linear interpolation (0 outside its times).
    ``resolve``: maps the file's path as written to the one to open."""
    t = np.asarray(times, dtype=np.float64)
    if spec.pulse[0] == "gaussian":
        _, t0, fwhm = spec.pulse
        return np.exp(-4.0 * math.log(2.0) * (t - t0) ** 2 / (fwhm * fwhm))
    path = spec.pulse[1]
    if resolve is not None:
        path = resolve(path)
    elif not os.path.isfile(path):
        raise FileNotFoundError(f"{KEY}.pulse.file: {path} not found")
    tt, vv = read_pulse_csv(path)
    return np.interp(t, tt, vv, left=0.0, right=0.0)


def power_density(power_watts, source_vector):
    """W -> W/m^3: the amplitude p with 2 pi p sum_i F1_i = power, F1 the source's load at unit amplitude."""
    total = math.fsum(float(v) for v in np.asarray(source_vector, dtype=np.float64))
    if not total > 0.0:
        raise ValueError(f"{KEY}: the source vector sums to {total!r} - no absorbing element carries the beam")
    return np.asarray(power_watts, dtype=np.float64) / (2.0 * math.pi * total)


def amplitudes(spec, times, source_vector, resolve=None):
    """The peak power densities p_k (W/m^3) of the steps that end at ``times``: power * pulse(t_k) / (2 pi sum F1)."""
    return power_density(spec.power * pulse_values(spec, times, resolve), source_vector)


def check_source_param(spec, name):
    """ValueError naming the parameter unless ``name`` (one of SOURCE_PARAMS) is a parameter of the source ``spec``."""
    if name not in SOURCE_PARAMS:
        raise ValueError(f"{name}: unknown source parameter (expected one of {', '.join(SOURCE_PARAMS)})")
    if spec is None:
        raise ValueError(f"{name}: the configuration has no volumetric source ({KEY})")
    if name == "source.depth" and not math.isfinite(spec.depth):
        raise ValueError(f"{name}: the source has no depth (uniform through the layer), so there is nothing to differentiate")
    if name.startswith("source.pulse.") and spec.pulse[0] != "gaussian":
        raise ValueError(f"{name}: the pulse comes from a file ({KEY}.pulse.file) and has no such parameter")


def tangent_coefficients(spec, names, times, F1, G_f, G_d, resolve=None):
    """{name: (n_steps, 3) array} of (c0, c1, c2) for the source parameters ``names`` at the steps that end at ``times``: the
    load of a tangent column in that parameter is c0 F1 + c1 G_f + c2 G_d = d(p_k F1)/dtheta, with
    p_k = P pulse_k / (2 pi sum F1) so that the configured power stays the discrete power:

        source.power        c0 = p_k / P
        source.fwhm         c0 = -p_k sum(G_f) / sum(F1),  c1 = p_k
        source.depth        c0 = -p_k sum(G_d) / sum(F1),  c2 = p_k
        source.pulse.t0     c0 = P / (2 pi sum F1) pulse_k 8 ln2 (t_k - t0) / w^2
        source.pulse.fwhm   c0 = P / (2 pi sum F1) pulse_k 8 ln2 (t_k - t0)^2 / w^3       (w = pulse.fwhm)

    G_f = dF1/dfwhm and G_d = dF1/ddepth come from the backend (HeatProblem.source_derivative); the sums are math.fsum's."""
    t = np.asarray(times, dtype=np.float64)
    total = math.fsum(float(v) for v in np.asarray(F1, dtype=np.float64))
    if not total > 0.0:
        raise ValueError(f"{KEY}: the source vector sums to {total!r} - no absorbing element carries the beam")
    pulse = pulse_values(spec, t, resolve)
    unit = 1.0 / (2.0 * math.pi * total)        # amplitude per watt
    p = spec.power * pulse * unit
    out = {}
    for name in names:
        check_source_param(spec, name)
        c = np.zeros((len(t), 3), dtype=np.float64)
        if name == "source.power":
            c[:, 0] = pulse * unit
        elif name == "source.fwhm":
            c[:, 0] = -p * (math.fsum(float(v) for v in np.asarray(G_f, dtype=np.float64)) / total)
            c[:, 1] = p
        elif name == "source.depth":
            c[:, 0] = -p * (math.fsum(float(v) for v in np.asarray(G_d, dtype=np.float64)) / total)
            c[:, 2] = p
        else:
            _, t0, w = spec.pulse
            k8 = 8.0 * math.log(2.0)
            if name == "source.pulse.t0":
                c[:, 0] = spec.power * unit * pulse * k8 * (t - t0) / (w * w)
            else:
                c[:, 0] = spec.power * unit * pulse * k8 * (t - t0) ** 2 / (w * w * w)
        out[name] = c
    return out
