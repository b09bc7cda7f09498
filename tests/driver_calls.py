"""Transcripts of what the Python drivers (heatflow_amd.driver.SimulationSession) ask of their backend, without a GPU.  TEST CODE:
it lives under tests/ and is never imported by heatflow_amd.

CallRecorder     a stand-in for HeatflowHIP, generic over __getattr__: logs every call with a digest of its arguments and answers
                 with zeros (ones for the source vectors) of the shapes the real backend returns
digest           scalars by repr, arrays by dtype, shape and SHA-256 of their bytes, dicts and sequences recursively, callables by
                 __qualname__
transcripts()    {case: [entries]} over the cases of tests/test_driver_calls_cpu.py (its docstring lists them); an entry is a
                 backend call "name(digests)", "-> keys" of a returned result, or "print: line" of what the driver printed (with
                 the wall-clock figures masked).  Only the public API of the session is used, so the same code records a
                 transcript at any commit (scripts/driver_calls_record.py) and compares it at any other.
"""
import contextlib
import copy
import hashlib
import io
import os
import re

import numpy as np
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "driver_calls.json")
SCALE, NSTEPS = 8.0, 3


def digest(x):
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return f"{a.dtype}{list(a.shape)}:{hashlib.sha256(a.tobytes()).hexdigest()}"
    if isinstance(x, dict):
        return "{" + ", ".join(f"{digest(k)}: {digest(v)}" for k, v in x.items()) + "}"
    if isinstance(x, (list, tuple)):
        if len(x) > 8 and all(isinstance(v, (int, float, np.integer, np.floating)) for v in x):
            return type(x).__name__ + ":" + digest(np.asarray(x))          # (a table's knots: one digest, not 64 reprs)
        body = ", ".join(digest(v) for v in x)
        return f"[{body}]" if isinstance(x, list) else f"({body})"
    if isinstance(x, (np.integer, np.floating, np.bool_)):
        return f"{type(x).__name__}({x.item()!r})"
    if callable(x):
        return f"<{x.__qualname__}>"
    return repr(x)


class CallRecorder:
    """Records the HeatflowHIP calls a session makes, with the digests of their arguments; the answers have the shapes of the
    real ones and hold zeros (ones for the source vectors, so that their sum is positive)."""

    def __init__(self):
        self.log = []
        self.n = self.tab_len = self.batch_nv = self.tangent_nv = 0
        self._mon = self._picard = self._heat = self._mt = 0         # records kept: monitors, Picard history, heat, derivatives
        self._heat_on = self._mt_on = False

    @property
    def calls(self):
        return [entry.split("(", 1)[0] for entry in self.log]

    def _stepped(self, nsteps, tangent=False):
        self._mon += nsteps
        self._picard += nsteps
        self._heat += nsteps if self._heat_on else 0
        self._mt += nsteps if tangent and self._mt_on else 0

    def _answer(self, name, a, k):
        nodes = lambda q: 0 if q is None else len(q)       # noqa: E731
        if name == "set_mesh":
            self.n, self.tab_len = len(a[0]), int(np.max(a[2])) + 1
            self.tangent_nv = self._mon = self._picard = self._heat = self._mt = 0
            self._heat_on = self._mt_on = False
        elif name in ("tangent_setup", "tangent_setup_dir"):
            self.tangent_nv, self._mt = next(v for v in (2, 4, 8, 16) if v >= int(a[0])), 0
        elif name in ("set_monitors", "clear_monitor_records"):
            self._mon = 0
        elif name in ("set_capacity_form", "clear_picard_history"):
            self._picard = 0
        elif name == "clear_heat_records":
            self._heat = 0
        elif name == "set_heat_records":
            self._heat_on = bool(a[0])
        elif name == "set_monitor_tangents":
            self._mt_on = bool(a[0])
        elif name == "batch_begin":
            self.batch_nv = int(a[0])
        elif name == "batch_end":
            self.batch_nv = 0
        elif name == "step":
            self._stepped(1)
            return 1, 0.0
        elif name == "run":
            ns = a[0].shape[0]
            self._stepped(ns)
            return np.zeros((ns, nodes(a[4]))), np.ones(ns, dtype=np.int32)
        elif name == "run_tangent":
            ns, nv, nn = a[0].shape[0], self.tangent_nv or 2, nodes(a[5])
            self._stepped(ns, tangent=True)
            return np.zeros((ns, nn)), np.ones(ns, dtype=np.int32), np.zeros((ns, nv, nn)), np.ones((ns, nv), dtype=np.int32)
        elif name == "batch_run":
            ns, nv, nn = a[0].shape[0], a[0].shape[2], nodes(a[4] if len(a) > 4 else None)
            self._batch_steps = ns
            out = np.zeros((ns, nv, nn)), np.ones((ns, nv), dtype=np.int32)
            if k.get("flux_nodes") is not None:
                comps = int(k.get("flux_components", 2))
                out += (np.zeros((ns, (comps & 1) + ((comps >> 1) & 1), nv, len(k["flux_nodes"]))),)
            return out
        elif name in ("get_state", "get_tangent", "tangent_load", "get_load"):
            return np.zeros(self.n)
        elif name in ("get_source", "get_source_derivative", "batch_get_source"):
            return np.ones(self.n)
        elif name == "sample":
            return np.zeros(nodes(a[0]))
        elif name == "flux_sample":
            return (np.zeros(len(a[0])) if k.get("want_z", True) else None,
                    np.zeros(len(a[0])) if k.get("want_r", True) else None)
        elif name == "amg_export":
            return None if k.get("into") is not None else np.arange(64, dtype=np.uint8)
        elif name == "export_pattern":
            return np.arange(32, dtype=np.uint8)
        elif name == "picard_history":
            return np.ones(self._picard, dtype=np.int32), np.zeros(self._picard)
        elif name == "picard_change":
            return 0.0
        elif name == "stored_heat":
            return np.zeros(self.tab_len)
        elif name == "get_heat":
            first = int(a[0]) if a else 0
            return np.zeros((max(self._heat - first, 0), self.tab_len))
        elif name == "monitor_now":
            return np.zeros((self.tab_len, 7))
        elif name == "monitor_count":
            return self._mon
        elif name == "get_monitors":
            first = int(a[0]) if a else 0
            count = self._mon - first if len(a) < 2 or a[1] is None else int(a[1])
            return np.zeros((max(count, 0), self.tab_len, 7))
        elif name == "monitor_tangent_count":
            return self._mt, self.tangent_nv
        elif name == "get_monitor_tangents":
            first = int(a[0]) if a else 0
            count = self._mt - first if len(a) < 2 or a[1] is None else int(a[1])
            return (np.zeros((max(count, 0), self.tab_len, self.tangent_nv, 5)),
                    (self._mon - self._mt + first + np.arange(max(count, 0))).astype(np.int32))
        elif name == "batch_get_monitors":
            return np.zeros((getattr(self, "_batch_steps", 0), self.batch_nv, self.tab_len, 7))
        return None

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def rec(*a, **k):
            self.log.append(f"{name}({', '.join([digest(v) for v in a] + [f'{q}={digest(v)}' for q, v in k.items()])})")
            return self._answer(name, a, k)
        return rec


# -- configurations and meshes ------------------------------------------------------------------------------------------------------
def config_names():
    """Every file of cfgs/ but konopkova.yaml (a stub: tests/test_mesh_geometry.py pins it as unparseable)."""
    return sorted(f[:-5] for f in os.listdir(os.path.join(ROOT, "cfgs")) if f.endswith(".yaml") and f != "konopkova.yaml")


def load(name, **timing):
    """The shipped configuration ``name`` on the coarse mesh, NSTEPS steps at its own dt; ``timing`` adds keys to its timing block."""
    from heatflow_amd.geometry import scale_mesh_sizes

    with open(os.path.join(ROOT, "cfgs", f"{name}.yaml")) as f:
        cfg = scale_mesh_sizes(yaml.safe_load(f), SCALE)
    dt = float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"])
    cfg["timing"] = dict(cfg["timing"], num_steps=NSTEPS, t_final=NSTEPS * dt, **timing)
    return cfg


_meshes = {}


def mesh_of(cfg):
    """(coords, tris, tags, material_tags) of the geometry of ``cfg``, built once per geometry."""
    from heatflow_amd.geometry import build_stack
    from heatflow_amd.mesh import Mesh

    key = repr(sorted((nm, [float(m[q]) for q in ("z", "r", "mesh")]) for nm, m in cfg["mats"].items()))
    if key not in _meshes:
        stack = build_stack(cfg)
        m = Mesh("mesh.msh", stack.bounds, stack.materials).build_mesh()
        _meshes[key] = (m.coords, m.tris, m.tags, dict(m.material_tags))
    return _meshes[key]


def varied(cfg, path, value):
    """A deep copy of ``cfg`` with the key at the dotted ``path`` set (a callable ``value`` maps the old one)."""
    out = copy.deepcopy(cfg)
    node, keys = out, path.split(".")
    for q in keys[:-1]:
        node = node.setdefault(q, {})
    node[keys[-1]] = value(node[keys[-1]]) if callable(value) else value
    return out


_MASK = re.compile(r"\d+\.\d{4} s")


class Transcript:
    """One case: a session on the mesh of ``cfg`` with a CallRecorder behind it, and the entries of what it did."""

    def __init__(self, cfg, **session_kw):
        from heatflow_amd.driver import SimulationSession

        self.backend = CallRecorder()
        self.entries = []
        self.session = SimulationSession(*mesh_of(cfg), backend=self.backend, **session_kw)

    def _do(self, call):
        start, out = len(self.backend.log), io.StringIO()
        with contextlib.redirect_stdout(out):
            res = call()
        self.entries += self.backend.log[start:]
        self.entries += ["print: " + _MASK.sub("* s", line) for line in out.getvalue().splitlines()]
        for r in ([] if res is None else res if isinstance(res, list) else [res]):
            self.entries.append("-> " + ", ".join(sorted(r)))
        return res

    def run(self, cfg, **kw):
        from heatflow_amd.geometry import build_stack, watcher_points

        return self._do(lambda: self.session.run(cfg, build_stack(cfg), watcher_points(cfg), **kw))

    def prepare(self, cfg):
        from heatflow_amd.geometry import build_stack

        return self._do(lambda: self.session.prepare(cfg, build_stack(cfg)))

    def run_batch(self, cfgs, **kw):
        from heatflow_amd.geometry import build_stack, watcher_points

        return self._do(lambda: self.session.run_batch(cfgs, [build_stack(c) for c in cfgs], watcher_points(cfgs[0]), **kw))

    def close(self):
        self._do(self.session.close)
        return self.entries


def mesh_digests():
    out = {}
    for name in ("geballe_with_diamond", "geballe_no_diamond"):
        coords, tris, tags, material_tags = mesh_of(load(name))
        out[name] = {"coords": digest(np.asarray(coords, dtype=np.float64)), "tris": digest(np.asarray(tris, dtype=np.int32)),
                     "tags": digest(np.asarray(tags, dtype=np.int32)), "material_tags": digest(dict(sorted(material_tags.items())))}
    return out


# -- the cases ----------------------------------------------------------------------------------------------------------------------
WD, ND = "geballe_with_diamond", "geballe_no_diamond"
K_SAMPLE = "mats.p_sample.k"


def _single(name):
    def case():
        cfg = load(name)
        t = Transcript(cfg)
        t.run(cfg)
        return t.close()
    return case


def _session_sequence():
    cfg = load(WD)
    t = Transcript(cfg)
    t.run(cfg)
    t.run(cfg)                                                       # reuse
    t.run(varied(cfg, K_SAMPLE, lambda k: k * 1.5))                  # re-value
    t.run(varied(cfg, K_SAMPLE, lambda k: k * 3.0))                  # hierarchy rebuilt
    dt = float(cfg["timing"]["t_final"]) / NSTEPS
    more = varied(varied(cfg, "timing.num_steps", NSTEPS + 2), "timing.t_final", (NSTEPS + 2) * dt)
    assert float(more["timing"]["t_final"]) / int(more["timing"]["num_steps"]) == dt
    t.run(more)                                                      # num_steps changed at the same dt: reuse
    t.run(varied(cfg, "timing.t_final", lambda tf: tf * 2.0))        # dt changed: a new problem
    return t.close()


def _prepare_then_run():
    cfg = load(WD)
    t = Transcript(cfg)
    t.prepare(cfg)
    t.run(cfg)
    return t.close()


def _shared_hierarchy(factor):
    def case():
        cfg = load(WD)
        first = Transcript(cfg)
        first.prepare(cfg)
        hierarchy = first.session.export_hierarchy()
        first.close()
        assert set(hierarchy) == {"blob", "k"}
        t = Transcript(cfg, hierarchy=hierarchy)
        t.run(varied(cfg, K_SAMPLE, lambda k: k * factor))
        t.run(varied(cfg, "timing.t_final", lambda tf: tf * 2.0))    # a later problem of the session builds its own
        return t.close()
    return case


def _read_flux_with_a_sink():
    cfg = load(ND)
    t = Transcript(cfg)
    fields = []
    t.run(cfg, read_flux=True, field_sink=lambda time, u: fields.append((time, u.shape)))
    assert len(fields) == NSTEPS
    return t.close()


def _run_with(name, edit=None, **kw):
    def case():
        cfg = load(name)
        if edit is not None:
            cfg = edit(cfg)
        t = Transcript(cfg)
        t.run(cfg, **kw)
        return t.close()
    return case


def _with_monitors(cfg):
    return varied(cfg, "monitors", {"coupler": {"material": "p_coupler", "above": 320.0}, "sample": {"material": "p_sample"}})


def _one_fwhm(cfg):
    out = varied(cfg, "heating.source.keep_line", True)
    del out["heating"]["source"]["fwhm"]
    return out


def _batch(name, edits, edit_all=None, before=None, **kw):
    def case():
        base = load(name)
        if edit_all is not None:
            base = edit_all(base)
        cfgs = []
        for e in edits:
            c = copy.deepcopy(base)
            for path, value in e.items():
                c = varied(c, path, value)
            cfgs.append(c)
        t = Transcript(base)
        if before is not None:
            before(t, base)
        t.run_batch(cfgs, **kw)
        return t.close()
    return case


SRC = "geballe_with_diamond_source"
CASES = {f"run {name}": _single(name) for name in config_names()}
CASES.update({
    "session: run, reuse, re-value, rebuild, more steps, new dt": _session_sequence,
    "prepare then run": _prepare_then_run,
    "shared hierarchy, k within 2x": _shared_hierarchy(1.5),
    "shared hierarchy, k beyond 2x": _shared_hierarchy(3.0),
    "read_flux with a field sink (step-wise loop)": _read_flux_with_a_sink,
    "two_sided": _run_with(WD, two_sided=True),
    "tangents p_sample, fwhm": _run_with(WD, tangents=["p_sample", "fwhm"]),
    "tangents k_r, k_z (aniso)": _run_with("geballe_with_diamond_aniso", tangents=["p_sample.k_r", "p_sample.k_z"]),
    "tangents thickness": _run_with(WD, tangents=["p_sample.thickness"]),
    "tangents rho_c, cv": _run_with(WD, tangents=["p_sample.rho_c", "p_ins.cv"]),
    # (the shipped source has keep_line: false, under which "fwhm" is refused: the heated line is kept here; the second case
    # drops the block's own fwhm, so that the beam takes heating.fwhm and "fwhm" carries both terms)
    "tangents under the source": _run_with("geballe_with_diamond_source_tangents",
                                           lambda c: varied(c, "heating.source.keep_line", True),
                                           tangents=["source.power", "source.fwhm", "fwhm"]),
    "tangents under the source, one fwhm": _run_with("geballe_with_diamond_source_tangents", _one_fwhm,
                                                     tangents=["source.power", "fwhm", "source.pulse.t0"]),
    "tangents under tables": _run_with("geballe_with_diamond_kT", lambda c: varied(c, "timing.table_tangents", True),
                                       tangents=["p_ins.k_power.exponent", "p_sample", "fwhm"]),
    "monitor_tangents": _run_with(WD, _with_monitors, tangents=["p_sample", "p_sample.rho_c"], monitor_tangents=True),
    "monitor_sigma": _run_with(WD, _with_monitors, tangents=["p_sample"], monitor_sigma={"p_sample.cv": 0.15, "fwhm": 0.1}),
    "batch: 2 columns, fwhm": _batch(WD, [{}, {"heating.fwhm": 9.0e-6}]),
    "batch: 4 columns, one k (affine)": _batch(WD, [{K_SAMPLE: k} for k in (3.2, 3.6, 4.0, 4.4)]),
    "batch: 2 columns, two k (per column)": _batch(WD, [{}, {K_SAMPLE: 4.4, "mats.p_ins.k": 12.0}]),
    "batch: 2 columns, a k beyond 2x (rebuild)": _batch(WD, [{K_SAMPLE: 3.0}, {K_SAMPLE: 10.0}],
                                                        before=lambda t, cfg: t.run(cfg)),
    "batch under source sweeps": _batch(SRC, [{}, {"heating.source.power": 0.4, "heating.source.depth": 4.0e-8}],
                                        lambda c: varied(c, "heating.source.sweeps", True)),
    "batch under sweep_monitors": _batch(WD, [{}, {"heating.fwhm": 9.0e-6}],
                                         lambda c: varied(_with_monitors(c), "timing.sweep_monitors", True)),
    "batch under sweep_tables": _batch("geballe_with_diamond_kT", [{}, {K_SAMPLE: 4.4}],
                                       lambda c: varied(c, "timing.sweep_tables", True)),
    "batch read_flux": _batch(ND, [{}, {"heating.fwhm": 9.0e-6}], read_flux=True),
    "single source run, then a batch under the source": _batch(SRC, [{}, {"heating.source.power": 0.4}],
                                                               lambda c: varied(c, "heating.source.sweeps", True),
                                                               before=lambda t, cfg: t.run(cfg)),
    "latent with monitors": _single("geballe_with_diamond_latent"),
})


def transcripts():
    return {name: case() for name, case in CASES.items()}
