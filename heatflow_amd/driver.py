"""Shared implementation of the ``run_simulation`` entry points.

``run_with_diamond.run_simulation`` / ``run_no_diamond.run_simulation`` keep the reference
signature (run_with_diamond.py:27, run_no_diamond.py:29):

    run_simulation(cfg, mesh_folder, rebuild_mesh=False, visualize_mesh=False,
                   output_folder=None, watcher_points=None, write_xdmf=True, suppress_print=False)

and the same side effects: mesh cache ``<mesh_folder>/mesh.msh`` + ``mesh_cfg.yaml`` (cfg copy
plus ``material_tags``, :194-230), ``<out>/used_config.yaml`` (:403-404), ``<out>/watcher_points.csv``
with columns ``time,<watcher names>`` (:510-515), default output folder
``sim_outputs/refactor_test`` (:405-409), ``FileNotFoundError`` when the cache is missing
(:219-226), ``ValueError`` for a bad ``watcher_points`` (:439) or heating CSV (:268-271),
``RuntimeError("No DOFs found ...")`` from the BC location (bc.py:105-106).

What differs by design: the mesh comes from heatflow_amd.mesh (no gmsh), assembly and the time
loop run on the GPU through libheatflow_hip.so, and a :class:`SimulationSession` keeps mesh,
sparsity pattern and mass matrix resident so a sweep re-values only what changed.
"""
from __future__ import annotations

import contextlib
import copy
import csv
import hashlib
import json
import os
import sys
import threading
import time
import warnings

import numpy as np
import yaml

_YAML_DUMPER = getattr(yaml, "CSafeDumper", yaml.SafeDumper)     # libyaml when PyYAML was built with it (10x faster)


def _dump_yaml(obj, f):
    yaml.dump(obj, f, Dumper=_YAML_DUMPER)


from .bc import P1Space, RowDirichletBC
from .geometry import check_thickness_name, stack_no_diamond, stack_with_diamond, thickness_velocity
from .heating import HeatingCurve
from .aniso import (CAPACITY_KINDS, DIRECTIONAL_HINT, aniso_tables, capacity_scale, check_capacity_names, check_config, refuse_aniso,
                    refuse_aniso_tables, split_param)
from .kappa_t import (capacity_form, check_capacity_form, check_sweep_tables, check_table_tangents, material_cv_table, picard_control,
                      refuse_enthalpy, material_table, picard_sweeps, refuse_tables,
                      refuse_tables_unless_swept, sweep_tables, table_keys, table_param,
                      table_tangents)
from .mesh import Mesh, load_mesh_arrays
from .monitors import (check_sigma, parse_monitors, problem_monitors, refuse_monitors_sweeps, uncertainty as monitor_uncertainty,
                       used_config as monitors_used_config, write_monitors_csv, write_uncertainty_csv)
from .source import (SOURCE_PARAMS, amplitudes as source_amplitudes, check_source_param, parse_source, refuse_source,
                     refuse_source_sweeps, source_block, tangent_coefficients)
from .solver import DEFAULT_MAX_IT, DEFAULT_RTOL, HeatProblem

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_quiet_lock = threading.Lock()
_quiet_depth = 0
_quiet_saved = None


@contextlib.contextmanager
def suppress_output(enabled):
    """Redirect stdout/stderr to devnull while ``enabled`` (reference run_with_diamond.py:18-25).
    Re-entrant across threads (concurrent sweep points): the first entrant redirects, the last one
    out restores."""
    global _quiet_depth, _quiet_saved
    if not enabled:
        yield
        return
    with _quiet_lock:
        if _quiet_depth == 0:
            sink = open(os.devnull, "w")
            _quiet_saved = (sys.stdout, sys.stderr, sink)
            sys.stdout = sys.stderr = sink
        _quiet_depth += 1
    try:
        yield
    finally:
        with _quiet_lock:
            _quiet_depth -= 1
            if _quiet_depth == 0:
                sys.stdout, sys.stderr, sink = _quiet_saved
                sink.close()
                _quiet_saved = None


def _resolve(path):
    """Heating file paths in the cfgs are relative to the repository root (cwd in the reference)."""
    if os.path.isabs(path) or os.path.isfile(path):
        return path
    alt = os.path.join(_PKG_ROOT, path)
    return alt if os.path.isfile(alt) else path


def _parse_watchers(watcher_points):
    if watcher_points is None:
        return [], []
    if isinstance(watcher_points, dict):
        return list(watcher_points.keys()), [tuple(v) for v in watcher_points.values()]
    if isinstance(watcher_points, list):
        return [pt["name"] for pt in watcher_points], [tuple(pt["coords"]) for pt in watcher_points]
    raise ValueError("watcher_points must be a dict or list of dicts")


_pending_mesh_writes = []


def flush_mesh_writes():
    """Wait for the mesh-cache files a ``prepare_mesh(..., defer_write=True)`` left to a background thread."""
    while _pending_mesh_writes:
        th, err = _pending_mesh_writes.pop()
        th.join()
        if err:
            raise err[0]


def prepare_mesh(cfg, mesh_folder, rebuild_mesh, stack, defer_write=False):
    """Build-and-cache or load the mesh.  Returns (coords, tris, tags, material_tags).  ``defer_write``: the cache files
    (``mesh.msh``, its sidecar, ``mesh_cfg.yaml``: 0.1 s of ASCII at 2e5 nodes) are written by a background thread while
    the caller goes on with the arrays - a sweep broadcasts them and never reads the files back; :func:`flush_mesh_writes`
    waits for them."""
    mesh_cfg_path = os.path.join(mesh_folder, "mesh_cfg.yaml")
    mesh_file_path = os.path.join(mesh_folder, "mesh.msh")
    if rebuild_mesh:
        mesh = Mesh(name="mesh.msh", boundaries=stack.bounds, materials=stack.materials)
        mesh.build_mesh()
        tag_map = {m.name: int(getattr(m, "_tag", -1)) for m in stack.materials}
        os.makedirs(mesh_folder, exist_ok=True)
        mesh_cfg = copy.deepcopy(cfg)
        mesh_cfg["material_tags"] = tag_map

        def write_files():
            with open(mesh_cfg_path, "w") as f:
                _dump_yaml(mesh_cfg, f)
            mesh.write(mesh_file_path)

        if defer_write:
            err = []

            def guarded():
                try:
                    write_files()
                except BaseException as e:      # noqa: BLE001 - re-raised by flush_mesh_writes
                    err.append(e)

            th = threading.Thread(target=guarded, name="heatflow-mesh-write", daemon=False)
            th.start()
            _pending_mesh_writes.append((th, err))
        else:
            write_files()
        return mesh.coords, mesh.tris, mesh.tags, tag_map
    missing = [nm for nm, p in (("mesh.msh", mesh_file_path), ("mesh_cfg.yaml", mesh_cfg_path)) if not os.path.isfile(p)]
    if missing:
        raise FileNotFoundError(f"Missing required file(s) in {mesh_folder}: {', '.join(missing)}")
    with open(mesh_cfg_path) as f:
        mesh_cfg = yaml.safe_load(f)
    tag_map = mesh_cfg["material_tags"]
    coords, tris, tags = load_mesh_arrays(mesh_file_path)
    return coords, tris, tags, tag_map


def time_scheme(cfg):
    """The time scheme a configuration asks for: ``timing.scheme`` = "backward_euler" (also when the key is absent: the
    reference's scheme) or "bdf2"; ValueError for anything else."""
    from .hip_backend import time_scheme_code

    name = (cfg.get("timing") or {}).get("scheme", "backward_euler")
    if name is None:
        name = "backward_euler"
    time_scheme_code(name)
    return name


def _with_scheme(cfg):
    """``cfg`` with the time scheme it runs with written out (``timing.scheme``), for used_config.yaml; with kappa(T) also
    ``timing.picard_sweeps`` and the tables that ran (``kappa_tables``: {material: {T0, dT, k}}); with cv(T) the same under
    ``rhoc_tables``: {material: {T0, dT, rho_cv}}, written only when a capacity table is set.  An anisotropic conductivity
    travels with its material (``mats.<name>.k_aniso``), so it is written exactly when it is set, and ``timing.aniso_tables``
    with the timing block, so only when the configuration sets it.  A volumetric
    source (``heating.source``, heatflow_amd.source) is written exactly when it is set too, with its defaults filled in, and so
    is a ``monitors`` block (heatflow_amd.monitors)."""
    out = dict(cfg)
    mon = parse_monitors(cfg)
    if mon is not None:
        out["monitors"] = monitors_used_config(mon)
    out["timing"] = dict(cfg.get("timing") or {}, scheme=time_scheme(cfg))
    src = parse_source(cfg)
    if src is not None:
        out["heating"] = dict(cfg["heating"], source=src.used_config())
    tables = {}
    for name, mat in sorted((cfg.get("mats") or {}).items()):
        t = material_table(name, mat) if isinstance(mat, dict) else None
        if t is not None:
            tables[name] = {"T0": float(t[0]), "dT": float(t[1]), "k": [float(v) for v in t[2]]}
    if tables:
        out["timing"]["picard_sweeps"] = picard_sweeps(cfg)
        out["kappa_tables"] = tables
    ctables = {}
    for name, mat in sorted((cfg.get("mats") or {}).items()):
        t = material_cv_table(name, mat) if isinstance(mat, dict) else None
        if t is not None:
            ctables[name] = {"T0": float(t[0]), "dT": float(t[1]), "rho_cv": [float(v) for v in t[2]]}
    if ctables:
        out["timing"]["picard_sweeps"] = picard_sweeps(cfg)
        out["rhoc_tables"] = ctables
    return out


def build_pattern_blob(coords, tris, tags, device_id=0):
    """The connectivity-derived tables of a mesh (CSR pattern, compressed column lists, row-gather assembly
    lists), built ONCE on this GPU and returned as a uint8 array: a sweep hands it to every solver session of
    every rank (``SimulationSession(..., pattern=blob)``), which then installs instead of rebuilding."""
    from .hip_backend import HeatflowHIP

    with HeatflowHIP(device_id) as be:
        be.set_mesh(coords, tris, tags)
        return be.export_pattern()


class SimulationSession:
    """A mesh resident on one GPU, reusable for many runs of the same geometry.

    ``run(cfg, ...)`` re-values the coefficient tables / matrices only when they differ from
    the previous run and re-tabulates the boundary values (fwhm, heating curve) on the host.
    """

    def __init__(self, coords, tris, tags, material_tags, *, device_id=0, backend=None, rtol=DEFAULT_RTOL,
                 max_it=DEFAULT_MAX_IT, assembly_mode=3, precond=1, pattern=None, hierarchy=None):
        self.coords = np.ascontiguousarray(coords, dtype=np.float64)
        self.tris = np.ascontiguousarray(tris, dtype=np.int32)
        self.tags = np.ascontiguousarray(tags, dtype=np.int32)
        self.material_tags = dict(material_tags)
        self.device_id, self.backend = device_id, backend
        self.rtol, self.max_it, self.assembly_mode = rtol, max_it, assembly_mode
        self.precond = precond           # 1 = multigrid-preconditioned CG (default), 0 = Jacobi-PCG
        self.pattern = pattern           # connectivity tables built once for this mesh (build_pattern_blob), or None
        # multigrid hierarchy another session built on this mesh: {"blob": HeatflowHIP.amg_export() output, "k": {cell tag:
        # conductivity it was built for}}; installed by the first problem this session creates instead of a host set-up
        self.hierarchy = hierarchy
        self.problem = None
        self._key = None
        self._source_F1 = None     # the resident problem's source vector, read back once per problem
        self._source_G = None      # its derivatives (G_f, G_d), read back once per problem by the first tangent run under it
        self._tree = None
        self._space = None
        self._dof_cache = {}

    def close(self):
        if self.problem is not None:
            self.problem.close()
            self.problem = None

    def export_hierarchy(self, into=None):
        """The multigrid hierarchy of the resident problem for other sessions on this mesh (``hierarchy=`` of their
        constructor): {"blob": uint8 array (or None when written ``into`` = (address, nbytes)), "k": {cell tag: conductivity}}."""
        if self.problem is None or self.precond != 1:
            raise RuntimeError("export_hierarchy: no resident problem with the multigrid preconditioner")
        return {"blob": self.problem.backend.amg_export(into=into), "k": dict(self._k_hier)}

    def prepare(self, cfg, stack):
        """Create the resident problem for ``cfg`` (mesh tables, matrices, multigrid hierarchy) without running a step."""
        num_steps = int(cfg["timing"]["num_steps"])
        dt = float(cfg["timing"]["t_final"]) / num_steps
        bcs = self._boundary_conditions(cfg, stack)
        tag_to_k, tag_to_rc = self._tables(stack)
        scheme = time_scheme(cfg)
        kt = self._kappa_tables(cfg, stack)
        an = self._aniso(stack)
        src = self._source(cfg, stack)
        mon = self._monitors(cfg)
        ant = aniso_tables(cfg)
        self._ensure_problem(self._problem_key(dt, tag_to_rc, bcs, scheme, kt, an, src, mon, ant), tag_to_k, tag_to_rc, dt, bcs,
                             float(cfg["heating"]["ic_temp"]), scheme, kt, an, src, mon, ant)

    def _tables(self, stack):
        tag_to_k = {self.material_tags[m.name]: m.properties["k"] for m in stack.materials}
        tag_to_rc = {self.material_tags[m.name]: m.properties["rho_cv"] for m in stack.materials}
        return tag_to_k, tag_to_rc

    def _aniso(self, stack):
        """{cell tag: (m_r, m_z)} of the materials of ``stack`` with a ``k_aniso`` block ({}: an isotropic configuration)."""
        return {self.material_tags[m.name]: m.properties["k_aniso"] for m in stack.materials if "k_aniso" in m.properties}

    def _source(self, cfg, stack):
        """dict(tags, fwhm, z0, depth) of a configuration with a ``heating.source`` block (HeatProblem's ``source=``), or None."""
        spec = parse_source(cfg)
        return None if spec is None else spec.problem_source(stack, self.material_tags)

    def _monitors(self, cfg):
        """{region: {"tags", "above"}} of a configuration with a ``monitors`` block (HeatProblem's ``monitors=``), or None."""
        spec = parse_monitors(cfg)
        return None if spec is None else problem_monitors(spec, self.material_tags)

    def _kappa_tables(self, cfg, stack):
        """(tables {tag: (T0, dT, values)}, Picard sweeps, capacity tables {tag: (T0, dT, values)}) of a kappa(T) / cv(T)
        configuration, or None."""
        tables = {self.material_tags[m.name]: m.properties["k_table"] for m in stack.materials if "k_table" in m.properties}
        ctables = {self.material_tags[m.name]: m.properties["rho_cv_table"] for m in stack.materials
                   if "rho_cv_table" in m.properties}
        if not (tables or ctables):
            check_capacity_form(cfg)
            return None
        form = {}
        if check_capacity_form(cfg) == "enthalpy":     # (absent / lagged: HeatProblem sees the arguments of before)
            tol, relax = picard_control(cfg)
            form = {"capacity_form": "enthalpy", "picard_tol": tol, "picard_relax": relax}
        return tables, picard_sweeps(cfg), ctables, form

    def _boundary_conditions(self, cfg, stack, two_sided=False):
        """[left, right, top, heated line(s)] of one configuration (reference run_with_diamond.py:343-374).  With a volumetric
        source (``heating.source``) and ``keep_line: false`` the three outer edges only: both coupler faces are free, and
        ``heating.file`` is not read."""
        ic_temp = float(cfg["heating"]["ic_temp"])
        src = parse_source(cfg)
        if src is not None and two_sided:
            refuse_source(cfg, "two_sided=True (a second heated line)")
        line = src is None or src.keep_line
        heat = HeatingCurve(_resolve(cfg["heating"]["file"]), ic_temp, float(cfg["heating"]["fwhm"])) if line else None
        if self._space is None:
            self._space = P1Space(self.coords)
        V = self._space

        def located(location, value, **kw):
            # the DOF set of an edge / line depends on the mesh and the location arguments only: located once per session
            key = (location,) + tuple(sorted(kw.items()))
            if key not in self._dof_cache:
                self._dof_cache[key] = RowDirichletBC(V, location, value=value, **kw).row_dofs
            return RowDirichletBC(V, location, value=value, row_dofs=self._dof_cache[key], **kw)

        bcs = [
            located("left", ic_temp),
            located("right", ic_temp),
            located("top", ic_temp),      # named bottom_bc in the reference, location 'top'
        ]
        if line:
            bcs.append(located("x", heat.gaussian, coord=float(stack.heated_z), length=abs(stack.r_sample) * 2, center=0.0))
        self._heats = [heat] if line else []   # the heated lines' curves, by position after the three edges (fwhm tangents)
        if two_sided:
            # EXTENSION without a reference implementation (BASELINE config 4 "konopkova two-sided",
            # SURVEY 8d C4): a second Gaussian Dirichlet line on the outer face of the o-side coupler,
            # driven by the CSV's `oside` column with the same offset-to-ic_temp convention.
            heat_o = HeatingCurve(_resolve(cfg["heating"]["file"]), ic_temp, float(cfg["heating"]["fwhm"]), column="oside")
            bcs.append(located("x", heat_o.gaussian, coord=float(stack.heated_z_oside), length=abs(stack.r_sample) * 2, center=0.0))
            self._heats.append(heat_o)
        return bcs

    def _problem_key(self, dt, tag_to_rc, bcs, scheme="backward_euler", kt=None, an=None, src=None, mon=None, ant=False, bt=False):
        # the resident problem is reusable only for exactly the same Dirichlet DOF sets, in the same order, and time scheme
        # (and kappa(T) tables and Picard sweeps, or anisotropy multipliers, when a configuration has them)
        key = (dt, tuple(sorted(tag_to_rc.items())),
               tuple(hashlib.sha1(np.ascontiguousarray(b.row_dofs, dtype=np.int64).tobytes()).hexdigest() for b in bcs),
               scheme)
        if kt is not None:
            key += (tuple((t, float(v[0]), float(v[1]), tuple(float(x) for x in v[2])) for t, v in sorted(kt[0].items())), kt[1])
            if kt[2]:
                key += (tuple((t, float(v[0]), float(v[1]), tuple(float(x) for x in v[2])) for t, v in sorted(kt[2].items())),)
            if len(kt) > 3 and kt[3]:
                key += (("capacity_form",) + tuple(sorted(kt[3].items(), key=lambda q: q[0])),)
        if an:
            key += (("k_aniso",) + tuple(sorted(an.items())),)
        if src:
            key += (("source", tuple(src["tags"]), src["fwhm"], src["z0"], src["depth"]),)
        if mon:
            key += (("monitors",) + tuple((region, tuple(r["tags"]), r["above"]) for region, r in mon.items()),)
        if ant:                  # timing.aniso_tables: the context's switch is set when the problem is made
            key += (("aniso_tables",),)
        if bt:                   # timing.sweep_tables: run_batch sets the context's switch on the problem it opens its batch on
            key += (("sweep_tables",),)
        return key

    def _ensure_problem(self, key, tag_to_k, tag_to_rc, dt, bcs, ic_temp, scheme="backward_euler", kt=None, an=None, src=None,
                        mon=None, ant=False):
        """The resident HeatProblem for ``key`` (built if absent), its operator valued for ``tag_to_k``."""
        if self.problem is None or key != self._key:
            self.close()
            print("Assigning material properties...")
            shared = self.hierarchy if (self.hierarchy is not None and self.precond == 1) else None
            self.problem = HeatProblem(self.coords, self.tris, self.tags, tag_to_k, tag_to_rc, dt, bcs, ic_temp,
                                       backend=self.backend, device_id=self.device_id, rtol=self.rtol,
                                       max_it=self.max_it, assembly_mode=self.assembly_mode, precond=self.precond,
                                       amg_reuse=True, pattern=self.pattern, amg=shared["blob"] if shared else None,
                                       scheme=scheme, **({"kappa_tables": kt[0], "picard": kt[1]} if kt else {}),
                                       **({"rhoc_tables": kt[2]} if kt and kt[2] else {}),
                                       **(kt[3] if kt and len(kt) > 3 else {}),
                                       **({"k_aniso": an} if an else {}), **({"source": src} if src else {}),
                                       **({"monitors": mon} if mon else {}), **({"aniso_tables": True} if ant else {}))
            self._key = key
            self._source_F1 = None
            self._source_G = None
            self._k = dict(tag_to_k)
            # conductivities the multigrid levels were built for: this problem's, or those of the session that shared them
            self._k_hier = dict(shared["k"]) if shared else dict(tag_to_k)
            self.hierarchy = None                    # a later problem of this session (other dt / Dirichlet set) builds its own
            if shared and set(self._k_hier) == set(tag_to_k):
                drift = max(max(tag_to_k[t] / self._k_hier[t], self._k_hier[t] / tag_to_k[t]) for t in tag_to_k)
                if drift > 2.0:                      # too far from this point's operator to be a good frozen hierarchy: rebuild
                    self.problem.backend.set_precond(1, False)
                    self.problem.set_materials(tag_to_k, tag_to_rc)
                    self.problem.backend.set_precond(1, True)
                    self._k_hier = dict(tag_to_k)
            print("Material properties assigned.")
            return
        self.problem.bcs = bcs
        if tag_to_k != self._k:
            self._revalue(tag_to_k, tag_to_rc)

    def _revalue(self, tag_to_k, tag_to_rc, allow_rebuild=True):
        # re-value A on the resident pattern; the frozen coarse levels stay a good preconditioner
        # while no conductivity moved by more than 2x from the values they were built for
        # (measured: 3.8 -> 60 W/m/K triples the iteration count), beyond that rebuild them
        drift = max(max(tag_to_k[t] / self._k_hier[t], self._k_hier[t] / tag_to_k[t]) for t in tag_to_k)
        if drift > 2.0 and self.precond == 1 and allow_rebuild:
            self.problem.backend.set_precond(1, False)
            self.problem.set_materials(tag_to_k, tag_to_rc)
            self.problem.backend.set_precond(1, True)
            self._k_hier = dict(tag_to_k)
        else:
            self.problem.set_materials(tag_to_k, tag_to_rc)
        self._k = dict(tag_to_k)

    def _watcher_nodes(self, watcher_points):
        names, coords_w = _parse_watchers(watcher_points)
        if not names:
            return names, None
        from .solver import nearest_nodes
        return names, nearest_nodes(self.coords, coords_w)

    def run_batch(self, cfgs, stacks, watcher_points=None, read_flux=False):
        """``len(cfgs)`` in (2, 4, 8, 16) simulations of this mesh advanced together (hf_batch_*): the points of a
        sweep that share geometry, time stepping and rho_c; they may differ in the boundary values (fwhm,
        heating curve: one shared operator) and in the conductivities (one operator per column, shared
        frozen multigrid hierarchy).  ``read_flux`` adds run_no_diamond's per-step gradient projection for every
        column (hf_batch_run_flux).  Returns one result dict per configuration, as :meth:`run` does.
        Under ``heating.source.sweeps: true`` the configurations may carry a ``heating.source`` block: they must
        agree on its ``material`` list, ``face`` and ``keep_line`` and may differ in ``power``, the beam's ``fwhm``, ``depth`` and
        ``pulse``; the batch gets a source of its own (hf_batch_set_source) with one amplitude column per configuration.  Under
        ``timing.sweep_monitors: true`` they may carry a ``monitors`` block, the same in all of them; every result then has
        ``monitors`` as :meth:`run` returns it.  A mismatch is a ValueError naming what differs.
        Under ``timing.sweep_tables: true`` the configurations may carry kappa(T) / cv(T) keys: they must agree
        on every table and on ``picard_sweeps: 1`` and may differ in the boundary values and in the constants of the materials
        without a conductivity table; the batch opens with per-column operators that every step re-values on the GPU, each
        column at its own temperatures (hf_set_batch_tables, hf_batch_set_column_kappa)."""
        nv = len(cfgs)
        for c in cfgs:
            refuse_enthalpy(c, "run_batch (the batched loop)")
            check_sweep_tables(c, "run_batch (the batched loop)")
            refuse_tables_unless_swept(c, "run_batch (the batched loop)")
            refuse_source_sweeps(c, "run_batch (the batched loop)")
            refuse_monitors_sweeps(c, "run_batch (the batched loop)")
        if nv not in (2, 4, 8, 16):
            raise ValueError("run_batch: 2, 4, 8 or 16 configurations at a time")
        specs = [parse_source(c) for c in cfgs]
        if any(sp is not None for sp in specs):
            if any(sp is None for sp in specs):
                raise ValueError("run_batch: some configurations have a heating.source block and some have none")
            for what, get in (("material", lambda sp: sp.materials), ("face", lambda sp: sp.face),
                              ("keep_line", lambda sp: sp.keep_line)):
                for j, sp in enumerate(specs):
                    if get(sp) != get(specs[0]):
                        raise ValueError(f"run_batch: the configurations must share heating.source.{what} "
                                         f"(configuration 0 has {get(specs[0])!r}, configuration {j} has {get(sp)!r})")
            z0s = [sp.z0(st) for sp, st in zip(specs, stacks)]
            if any(z != z0s[0] for z in z0s):
                raise ValueError(f"run_batch: the configurations must share the absorbing face's z (heating.source: z0 = {z0s!r})")
        mon_specs = [parse_monitors(c) for c in cfgs]
        for j, m in enumerate(mon_specs):
            if m != mon_specs[0]:
                raise ValueError(f"run_batch: the configurations must share the monitors block (configuration {j} differs from "
                                 "configuration 0)")
        mon = self._monitors(cfgs[0])
        # tables (timing.sweep_tables): the same in every configuration, material by material
        tabled = [bool(table_keys(c)) for c in cfgs]
        if any(tabled):
            if not all(sweep_tables(c) for c in cfgs):
                raise ValueError("run_batch: the configurations must share timing.sweep_tables")
            names = sorted({str(nm) for c in cfgs for nm in (c.get("mats") or {})})
            for nm in names:
                per = []
                for c in cfgs:
                    mat = (c.get("mats") or {}).get(nm)
                    tabs = (material_table(nm, mat), material_cv_table(nm, mat)) if isinstance(mat, dict) else (None, None)
                    per.append(tuple(None if t is None else (float(t[0]), float(t[1]), tuple(float(v) for v in t[2])) for t in tabs))
                for j, t in enumerate(per):
                    if t != per[0]:
                        raise ValueError(f"run_batch: the configurations must share every table under timing.sweep_tables: the tables "
                                         f"of material {nm} differ between configuration 0 and configuration {j}")
        t_start = time.time()
        cfg0 = cfgs[0]
        num_steps = int(cfg0["timing"]["num_steps"])
        dt = float(cfg0["timing"]["t_final"]) / num_steps
        ic_temp = float(cfg0["heating"]["ic_temp"])
        scheme = time_scheme(cfg0)
        cols = []
        for cfg, stack in zip(cfgs, stacks):
            bcs = self._boundary_conditions(cfg, stack)
            tk, trc = self._tables(stack)
            key = self._problem_key(float(cfg["timing"]["t_final"]) / int(cfg["timing"]["num_steps"]), trc, bcs, time_scheme(cfg),
                                    None, self._aniso(stack))
            cols.append((bcs, tk, trc, key))
            if int(cfg["timing"]["num_steps"]) != num_steps or float(cfg["heating"]["ic_temp"]) != ic_temp or key != cols[0][3]:
                raise ValueError("run_batch: the configurations must share time stepping (and scheme), ic_temp, rho_c, the Dirichlet sets "
                                 "and the anisotropy multipliers (k_aniso)")
        percol = any(c[1] != cols[0][1] for c in cols)
        mid = cols[nv // 2]
        # conductivities that differ between the columns; a single one (sweep_test.py's kappa_sample list) makes
        # the operators an affine family A + (kappa_j - kappa_ref) A1: two shared matrices instead of nv
        varying = [t for t in mid[1] if any(c[1][t] != mid[1][t] for c in cols)]
        affine = percol and len(varying) == 1
        kt = self._kappa_tables(cfgs[nv // 2], stacks[nv // 2]) if any(tabled) else None
        if kt is not None:       # under tables every column has its own operator, re-valued by the batch itself
            percol, affine = True, False
        # the batch's problem carries the monitors' table and no source of its own (the batch gets one: hf_batch_begin refuses the
        # context's); a resident problem that differs by its source alone (a single run before, or prepare) gives the source up
        an_mid = self._aniso(stacks[nv // 2])
        key = self._problem_key(dt, mid[2], mid[0], scheme, kt, an_mid, None, mon, False, kt is not None)
        if specs[0] is not None and self.problem is not None and self.problem.source and \
                self._key == self._problem_key(dt, mid[2], mid[0], scheme, None, an_mid, self.problem.source, mon):
            self.problem.backend.set_source(None)
            self.problem.source = None
            self._key, self._source_F1, self._source_G = key, None, None
        self._ensure_problem(key, mid[1], mid[2], dt, mid[0], ic_temp, scheme, kt, an_mid, None, mon)
        prob = self.problem
        be = prob.backend
        if percol and self.precond == 1:             # all columns share the hierarchy: keep every column within its range
            worst = max(max(max(c[1][t] / self._k_hier[t], self._k_hier[t] / c[1][t]) for t in c[1]) for c in cols)
            if worst > 2.0:
                be.set_precond(1, False)
                prob.set_materials(mid[1], mid[2])
                be.set_precond(1, True)
                self._k_hier, self._k = dict(mid[1]), dict(mid[1])
        times = (np.arange(num_steps) + 1) * dt
        g_all = np.empty((num_steps, len(prob.bc_dofs), nv), dtype=np.float64)
        tabulated = {}                                   # columns with the same boundary definition share one table
        for j, (bcs, _, _, _) in enumerate(cols):
            h = cfgs[j]["heating"]
            if len(bcs) > 3:
                sig = (str(h["file"]), float(h["ic_temp"]), float(h["fwhm"]), len(bcs))
            else:                                        # keep_line: false - the three outer edges only, no heating file
                sig = (None, float(h["ic_temp"]), None, len(bcs))
            if sig not in tabulated:
                prob.bcs = bcs
                for bc in bcs:
                    bc.update(0.0)
                tabulated[sig] = np.stack([prob.bc_values(t, bcs[3:]) for t in times])
            g_all[:, :, j] = tabulated[sig]
        prob.bcs = cols[-1][0]
        names, nodes = self._watcher_nodes(watcher_points)
        if affine and mid[1] != self._k:
            self._revalue(mid[1], mid[2], allow_rebuild=False)     # the context's operator is the reference of the family
        flux0 = FluxSampler(self.coords) if read_flux else None
        if flux0 is not None and not getattr(prob, "_flux_ready", False):
            print("Setting up radial heat flux sampling...")
            be.flux_setup()                    # once per mesh: the unit-coefficient mass matrix does not depend on kappa
            prob._flux_ready = True
        if kt is not None:
            be.set_state(np.full(prob.n, ic_temp))       # (a resident problem may stand at the end of an earlier run)
            be.set_batch_tables(True)
        be.batch_begin(nv, per_column_operator=2 if affine else (1 if percol else 0))
        try:
            if kt is not None:   # the constants of the materials without a conductivity table, column by column
                free = sorted(t for t in mid[1] if t not in kt[0])
                for j, (_, tk, _, _) in enumerate(cols):
                    be.batch_set_column_kappa(j, free, [tk[t] for t in free])
            elif affine:
                be.batch_set_affine(varying, [c[1][varying[0]] - mid[1][varying[0]] for c in cols])
            elif percol:
                for j, (_, tk, trc, _) in enumerate(cols):
                    if tk != self._k:
                        self._revalue(tk, trc, allow_rebuild=False)
                    be.batch_load_column(j)
            for j in range(nv):
                be.batch_set_state(j, np.full(prob.n, ic_temp))
            if specs[0] is not None:     # the batch's own source; W -> W/m^3 per step and column, from each column's own integral
                be.batch_set_source([int(self.material_tags[m]) for m in specs[0].materials], [sp.fwhm for sp in specs], z0s[0],
                                    [sp.depth for sp in specs])
                amp, vectors = np.empty((num_steps, nv), dtype=np.float64), {}
                for j, sp in enumerate(specs):
                    if (sp.fwhm, sp.depth) not in vectors:       # columns with the same (fwhm, depth) download once
                        vectors[(sp.fwhm, sp.depth)] = be.batch_get_source(j)
                    amp[:, j] = source_amplitudes(sp, times, vectors[(sp.fwhm, sp.depth)], _resolve)
                be.batch_set_source_amplitudes(amp)
            if mon:
                be.batch_set_monitors(True)
            print("Beginning loop...")
            t_loop = time.time()
            if flux0 is None:
                samples, iters = be.batch_run(g_all, self.rtol, 0.0, self.max_it, nodes)
            else:                              # d/dr only, as the single run (run_no_diamond.py:553-566 reads nothing else)
                samples, iters, grad = be.batch_run(g_all, self.rtol, 0.0, self.max_it, nodes, flux_nodes=flux0.nodes,
                                                    flux_components=2, flux_rtol=self.rtol, flux_max_it=5000)
            loop_time = time.time() - t_loop
            records = be.batch_get_monitors() if mon else None      # [step, column, tag, field]
        finally:
            be.batch_end()
        fluxes = [None] * nv
        if flux0 is not None:
            for j in range(nv):
                fluxes[j] = flux0 if j == 0 else flux0.clone()
                for s, t in enumerate(times):
                    fluxes[j].record_sampled(t, grad[s, 0, j])
        print(f"Simulation progress: 100% (step {num_steps}/{num_steps}) | {nv} runs together | Avg time/step: "
              f"{loop_time / num_steps:.4f} s | PCG iterations/step: mean {np.mean(iters):.0f}, max {int(np.max(iters))}")
        return [{"times": times.copy(), "watcher_names": names,
                 "watchers": {nm: samples[:, j, k].copy() for k, nm in enumerate(names)},
                 "iters": iters[:, j].copy(), "loop_time": loop_time / nv, "startup_time": (t_loop - t_start) / nv,
                 "n_dof": prob.n, "dt": dt, "flux": fluxes[j], "batch": nv,
                 **({"monitors": prob._combine_monitors(records[:, j])} if mon else {})} for j in range(nv)]

    def run(self, cfg, stack, watcher_points=None, field_sink=None, read_flux=False, two_sided=False, tangents=None,
            monitor_tangents=False, monitor_sigma=None):
        """One simulation (reference loop run_with_diamond.py:456-504).  Returns a dict with
        ``times``, ``watchers`` {name: array}, ``iters``, timing numbers.  ``read_flux`` adds the
        per-step gradient projection of run_no_diamond.py:543-566 (``flux`` entry of the result).
        ``tangents`` = parameter names (material names - the derivative with respect to that material's conductivity
        k -, "<material>.k_r" / "<material>.k_z" / "<material>.k" - its radial, its axial conductivity in W/m/K, or the
        scalar k of both with the ratio of ``k_aniso`` kept; on isotropic materials the derivatives at m = (1, 1) -,
        "<material>.thickness" - the layer thickness ``mats.<material>.z`` in metres, the nodes of this session's mesh moving
        with the stack (geometry.thickness_velocity) -, "<material>.rho_c" / "<material>.cv" / "<material>.rho" -
        the material's rho * cv in J/m^3/K, its cv or its rho (one of the three per material) -, and / or "fwhm"
        of the heating profile) adds ``tangents`` {param: {watcher: d watcher / d param}} and ``tangent_iters`` (HeatProblem.run_tangent; not with a field sink or the flux projection).
        A ``heating.source`` block (heatflow_amd.source) drives the run by absorbed laser power, the field sink and the flux
        projection included; not with ``two_sided``, and with ``tangents`` only under ``heating.source.tangents: true`` (DESIGN.md
        3.19).  Then ``tangents``, ``monitor_tangents`` and ``monitor_sigma`` take the names above and the source's own -
        "source.power" (W), "source.fwhm", "source.depth" (m), "source.pulse.t0", "source.pulse.fwhm" (s) -; ValueError naming the
        parameter for "source.depth" on a block without ``depth``, "source.pulse.*" on a file pulse, "<material>.thickness" under
        a source (its load depends on the node positions; that term is not formed) and "fwhm" with ``keep_line: false`` (there is
        no heated line; the beam's width is "source.fwhm"), and for any "source.*" name without a source.  A ``monitors`` block (heatflow_amd.monitors) adds
        ``monitors`` {region: {field: one value per step}} to the result, whichever way the steps are taken.
        ``monitor_tangents`` (with ``tangents`` and a ``monitors`` block) adds ``monitor_tangents``
        {param: {region: {field: d field / d param per step}}}.  ``monitor_sigma`` = {param: relative one-sigma}, the names the
        ones ``tangents`` accepts and the values from fit.get_param, implies those tangent columns and the derivatives and adds
        ``monitor_uncertainty`` {region: {field: sqrt(sum_q (d field / d theta_q sigma_q theta_q)^2) per step}}."""
        t_start = time.time()
        if monitor_tangents or monitor_sigma is not None:
            arg = "monitor_sigma" if monitor_sigma is not None else "monitor_tangents"
            if parse_monitors(cfg) is None:
                raise ValueError(f"{arg}: the configuration has no monitors block (heatflow_amd.monitors)")
            sigma = check_sigma(monitor_sigma) if monitor_sigma is not None else {}
            tangents = list(tangents or ()) + [q for q in sigma if q not in (tangents or ())]
            if not tangents:
                raise ValueError("monitor_tangents: no parameter (tangents= names the columns)")
            if len(tangents) > 16:
                raise ValueError(f"{arg}: {len(tangents)} tangent columns (at most 16 per run)")
            monitor_tangents = True
        spec = parse_source(cfg)
        if spec is not None and tangents and not spec.tangents:
            refuse_source(cfg, "tangents=")
        for p in tangents or ():     # the source's own names, and the names a source rules out, before any problem is made
            if p in SOURCE_PARAMS or p.startswith("source."):
                try:
                    check_source_param(spec, p)
                except ValueError as e:
                    raise ValueError(f"tangents: {e}") from None
            elif spec is not None and p == "fwhm" and not spec.keep_line:
                raise ValueError("tangents: parameter 'fwhm': the heated line is off (heating.source.keep_line: false); the beam's "
                                 "width is 'source.fwhm'")
            elif spec is not None and p.endswith(".thickness"):
                raise ValueError(f"tangents: parameter {p!r}: a layer thickness under a volumetric source (heating.source) is not "
                                 "supported (the source's load depends on the node positions, and that term is not formed)")
        t_final = float(cfg["timing"]["t_final"])
        num_steps = int(cfg["timing"]["num_steps"])
        dt = t_final / num_steps
        ic_temp = float(cfg["heating"]["ic_temp"])
        bcs = self._boundary_conditions(cfg, stack, two_sided)
        varying = bcs[3:]
        tag_to_k, tag_to_rc = self._tables(stack)
        scheme = time_scheme(cfg)
        if tangents:
            refuse_enthalpy(cfg, "monitor_sigma=" if monitor_sigma is not None else "tangents=")
        kt = self._kappa_tables(cfg, stack)
        enth = kt is not None and bool(kt[3])        # timing.capacity_form: enthalpy
        if tangents:             # both kinds: timing.aniso_tables covers the forward run only, with timing.table_tangents too
            refuse_aniso_tables(cfg, "monitor_sigma" if monitor_sigma is not None else "tangents")
        tab_on = kt is not None and bool(tangents) and table_tangents(cfg)   # timing.table_tangents
        if kt is not None and tangents and not tab_on:
            refuse_tables(cfg, "tangents")
        if tab_on:
            if monitor_tangents:
                raise ValueError(("monitor_sigma" if monitor_sigma is not None else "monitor_tangents")
                                 + ": monitor derivatives together with timing.table_tangents are not supported")
            check_table_tangents(cfg, "tangents", tangents)
            for p in tangents:       # the names of the tables' parameters, before any problem is made
                try:
                    tp = None if p == "fwhm" else table_param(cfg, p)
                except ValueError as e:
                    raise ValueError(f"tangents: {e}") from None
                mat, _, suffix = p.rpartition(".")
                if tp is None and suffix in ("k_r", "k_z") and self.material_tags.get(mat) in kt[0]:
                    raise ValueError(f"tangents: parameter {p!r}: {mat!r} carries a conductivity table (its parameters are "
                                     f"{mat}.k or {mat}.k_power.exponent, or {mat}.k_table.scale)")
        an = self._aniso(stack)
        if an and tangents:      # a bare name means the isotropic k: an anisotropic material is named by direction
            refuse_aniso(cfg, "a tangent with respect to the conductivity of an anisotropic material", set(tangents),
                         DIRECTIONAL_HINT)
        src = self._source(cfg, stack)
        mon = self._monitors(cfg)
        ant = aniso_tables(cfg)
        key = self._problem_key(dt, tag_to_rc, bcs, scheme, kt, an, src, mon, ant)
        fresh = self.problem is None or key != self._key
        self._ensure_problem(key, tag_to_k, tag_to_rc, dt, bcs, ic_temp, scheme, kt, an, src, mon, ant)
        if not fresh:
            self.problem.set_state(ic_temp)
            self.problem.iters = []
        prob = self.problem
        if mon and not fresh:    # the records of this run only
            prob.clear_monitor_history()
        if enth:                 # the sweeps and changes of this run only; with monitors the stored heat per step, for `energy`
            if not fresh:
                prob.clear_picard_history()
            if mon:
                prob.clear_heat_history()
                prob.record_heat()
        amp = None
        if spec is not None:     # W -> W/m^3 per step, from the discrete source's own integral
            if self._source_F1 is None:
                self._source_F1 = prob.source_vector()
            amp = source_amplitudes(spec, (np.arange(num_steps) + 1) * dt, self._source_F1, _resolve)
        names, nodes = self._watcher_nodes(watcher_points)

        flux = FluxSampler(self.coords) if read_flux else None
        if flux is not None and not getattr(prob, "_flux_ready", False):
            print("Setting up radial heat flux sampling...")
            prob.backend.flux_setup()          # once per mesh: the unit-coefficient mass matrix does not depend on kappa
            prob._flux_ready = True
        print("Beginning loop...")
        t_loop = time.time()
        tangent_out, extra = None, {}
        if tangents:
            if field_sink is not None or flux is not None:
                raise ValueError("tangents: not combined with a field sink or the read-flux projection")
            params = list(tangents)
            try:
                check_capacity_names(params)
            except ValueError as e:
                raise ValueError(f"tangents: {e}") from None
            cond, bnd, shp, cap, cscale, srcp, tabs = [], {}, {}, {}, {}, {}, {}
            for j, p in enumerate(params):
                try:
                    tp = table_param(cfg, p) if tab_on and p != "fwhm" else None
                except ValueError as e:
                    raise ValueError(f"tangents: {e}") from None
                if tp is not None:       # a parameter of a material's table: a derivative table on the table's own grid
                    cond.append([])
                    tabs[j] = {tp[1]: {self.material_tags[tp[0]]: tp[2]}}
                elif p in SOURCE_PARAMS:
                    cond.append([])
                    srcp[j] = p
                elif p == "fwhm":
                    cond.append([])
                    bnd[j] = {3 + q: h.gaussian_dfwhm for q, h in enumerate(self._heats)}
                    if spec is not None and "fwhm" not in source_block(cfg):   # the beam takes heating.fwhm too: both terms
                        srcp[j] = "source.fwhm"
                elif p in self.material_tags:
                    cond.append([self.material_tags[p]])
                else:
                    try:
                        mat, kind = split_param(p)
                    except ValueError as e:
                        raise ValueError(f"tangents: {e}") from None
                    if kind is None or mat not in self.material_tags:
                        raise ValueError(f"tangents: unknown parameter {p!r} (a material name, <material>.k_r, "
                                         "<material>.k_z, <material>.k, <material>.thickness or 'fwhm')")
                    if kind == "t":      # a layer thickness: the nodes of this session's mesh move with the stack of ``cfg``
                        try:
                            check_thickness_name(cfg, mat, p)
                        except ValueError as e:
                            raise ValueError(f"tangents: {e}") from None
                        cond.append([])
                        shp[j] = thickness_velocity(cfg, mat, self.coords[:, 0])
                    elif kind in CAPACITY_KINDS.values():      # a column in rho_c = rho cv of the material; cv and rho by the chain rule
                        if mat not in (cfg.get("mats") or {}):
                            raise ValueError(f"tangents: parameter {p!r}: no material {mat!r} in the configuration")
                        cond.append([])
                        cap[j] = [self.material_tags[mat]]
                        cscale[j] = capacity_scale(cfg["mats"][mat], kind)
                    else:
                        cond.append([(self.material_tags[mat], kind)])
            src_kw = {}
            if spec is not None:     # the opt-in: the source becomes differentiable, its own parameters get their columns
                src_cols = {}
                if srcp:
                    if self._source_G is None:
                        self._source_G = (prob.source_derivative("fwhm"), prob.source_derivative("depth"))
                    table = tangent_coefficients(spec, sorted(set(srcp.values())), (np.arange(num_steps) + 1) * dt, self._source_F1,
                                                 self._source_G[0], self._source_G[1], _resolve)
                    src_cols = {j: {"amplitude": table[p][:, 0], "fwhm": table[p][:, 1], "depth": table[p][:, 2]}
                                for j, p in srcp.items()}
                src_kw = {"source": src_cols, "source_amplitude": amp}
            times, samples, tsamp, iters, titers = prob.run_tangent(num_steps, nodes, conductivity=cond, boundary=bnd,
                                                                    time_varying=varying, **({"shape": shp} if shp else {}),
                                                                    **({"capacity": [cap.get(j, []) for j in range(len(params))]}
                                                                       if cap else {}),
                                                                    **({"monitor_tangents": True} if monitor_tangents else {}),
                                                                    **({"tables": tabs} if tab_on else {}),
                                                                    **src_kw)
            for j, f in cscale.items():
                if f != 1.0:
                    tsamp[:, j] *= f
            tangent_out = {p: {nm: tsamp[:, j, k] for k, nm in enumerate(names)} for j, p in enumerate(params)}
            if monitor_tangents:
                dhist = prob.monitor_tangent_history(scale=[cscale.get(j, 1.0) for j in range(len(params))])
                extra = {"monitor_tangents": {p: {region: {field: d[:, j] for field, d in f.items()} for region, f in dhist.items()}
                                              for j, p in enumerate(params)}}
                if monitor_sigma is not None:
                    from .fit import get_param
                    extra["monitor_uncertainty"] = monitor_uncertainty(extra["monitor_tangents"],
                                                                       {q: s * get_param(cfg, q) for q, s in sigma.items()})
        elif field_sink is None and flux is None:
            times, samples, iters = prob.run(num_steps, watcher_nodes=nodes, time_varying=varying,
                                             **({"source_amplitude": amp} if amp is not None else {}))
        else:  # step-wise: every field goes to the sink (visualisation) and / or through the flux projection
            for bc in bcs:
                bc.update(0.0)
            times, rows, iters = [], [], []
            for step in range(num_steps):
                t = (step + 1) * dt
                it, _ = prob.step(t, only=varying, **({"source_amplitude": float(amp[step])} if amp is not None else {}))
                if flux is not None:
                    prob.backend.flux_solve(self.rtol, 5000, want_z=False)          # d/dr only, on the device
                    flux.record_sampled(t, prob.backend.flux_sample(flux.nodes, want_z=False)[1])
                if field_sink is not None:
                    u = prob.state()
                    field_sink(t, u)
                    rows.append(u[nodes] if nodes is not None else np.zeros(0))
                else:
                    rows.append(prob.backend.sample(nodes) if nodes is not None else np.zeros(0))
                times.append(t)
                iters.append(it)
            times, samples, iters = np.array(times), np.array(rows), np.array(iters)
        loop_time = time.time() - t_loop
        print(f"Simulation progress: 100% (step {num_steps}/{num_steps}) | Avg time/step: {loop_time / num_steps:.4f} s"
              f" | PCG iterations/step: mean {np.mean(iters):.0f}, max {int(np.max(iters))}")
        mon_out, picard_out = None, {}
        if mon:
            mon_out = prob.monitor_history()
            if enth:             # every region's energy from the heat records: the stored heat the scheme conserves, tabled tags included
                heat = prob.heat_history()
                for region, r in mon.items():
                    mon_out[region]["energy"] = sum(heat[int(t)] for t in r["tags"])
        if enth:
            hist = prob.picard_history()
            picard_out = {"picard": {"sweeps": np.asarray(hist["sweeps"]), "change": np.asarray(hist["change"])}}
            tol = kt[3]["picard_tol"]
            if tol:
                late = np.flatnonzero((picard_out["picard"]["sweeps"] >= kt[1]) & (picard_out["picard"]["change"] > tol))
                if late.size:
                    warnings.warn(f"timing.picard_sweeps = {kt[1]}: step {int(late[0]) + 1} ended at the cap with a Picard change of "
                                  f"{picard_out['picard']['change'][late[0]]:.3g} K > timing.picard_tol = {tol:g} K "
                                  f"({late.size} such step(s); more sweeps or timing.picard_relax < 1 may help)", RuntimeWarning,
                                  stacklevel=2)
        return {
            "times": np.asarray(times), "watcher_names": names,
            "watchers": {nm: samples[:, k] for k, nm in enumerate(names)},
            "iters": np.asarray(iters), "loop_time": loop_time, "startup_time": t_loop - t_start,
            "n_dof": prob.n, "dt": dt, "flux": flux,
            **({"tangents": tangent_out, "tangent_iters": titers} if tangent_out is not None else {}),
            **({"monitors": mon_out} if mon else {}),
            **picard_out,
            **extra,
        }


class FluxSampler:
    """Bookkeeping of run_no_diamond's radial-gradient outputs (reference run_no_diamond.py):
    * smoothed: mean of d T/d r over the nodes with 0 < r <= 0.25 um that fall into each 0.2-um z bin
      (:494-513, :553-556) -> ``radial_gradient.csv`` (columns = bin centres, :603-608);
    * raw: d T/d r at the nodes on the axis (|r| <= 1e-12), ordered by z (:457-465, :559-566)
      -> ``radial_gradient_raw.csv`` (columns = their z, :611-617)."""

    DZ_BIN = 0.2e-6
    BAND = 0.25e-6
    R_TOL = 1e-12

    def __init__(self, coords):
        z, r = coords[:, 0], coords[:, 1]
        edges = np.arange(z.min(), z.max() + self.DZ_BIN, self.DZ_BIN)
        band = np.nonzero((r > 0.0) & (r <= self.BAND))[0]
        k = np.searchsorted(edges, z[band]) - 1
        ok = (k >= 0) & (k < len(edges) - 1)
        band, k = band[ok], k[ok]
        self.z_centres, self.groups = [], []
        for b in np.unique(k):
            self.z_centres.append(0.5 * (edges[b] + edges[b + 1]))
            self.groups.append(band[k == b])
        axis = np.nonzero(np.abs(r) <= self.R_TOL)[0]
        order = np.argsort(z[axis], kind="stable")
        self.axis_nodes = axis[order]
        self.axis_z = z[self.axis_nodes]
        self.times, self.rows, self.raw_rows = [], [], []
        # the only nodes whose gradient is ever read: band groups first, axis nodes last (hf_flux_sample order)
        self.nodes = np.concatenate(self.groups + [self.axis_nodes]).astype(np.int32) if self.groups else self.axis_nodes.astype(np.int32)
        self._cuts = np.cumsum([len(g) for g in self.groups])

    def clone(self):
        """An empty sampler of the same mesh (the node groups are shared, the recorded rows are not)."""
        import copy as _copy
        c = _copy.copy(self)
        c.times, c.rows, c.raw_rows = [], [], []
        return c

    def record(self, t, grad_r):
        """grad_r: the full nodal field."""
        self.record_sampled(t, np.asarray(grad_r)[self.nodes])

    def record_sampled(self, t, values):
        """values: d T/d r at ``self.nodes`` (what hf_flux_sample returns)."""
        self.times.append(float(t))
        parts = np.split(values, self._cuts) if len(self._cuts) else [values]
        self.rows.append([float(np.mean(p)) for p in parts[:len(self.groups)]])
        self.raw_rows.append(parts[-1].astype(float).tolist())

    @staticmethod
    def _write(path, times, columns, rows):
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["time"] + [repr(float(c)) for c in columns])
            for t, row in zip(times, rows):
                w.writerow([repr(t)] + [repr(v) for v in row])

    def write(self, folder):
        if self.rows:
            self._write(os.path.join(folder, "radial_gradient.csv"), self.times, self.z_centres, self.rows)
            self._write(os.path.join(folder, "radial_gradient_raw.csv"), self.times, self.axis_z, self.raw_rows)


def write_watcher_csv(path, times, names, watchers):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["time"] + list(names))
        for k, t in enumerate(times):
            w.writerow([repr(float(t))] + [repr(float(watchers[nm][k])) for nm in names])


class _FieldWriter:
    """``output.xdmf`` time series (reference :414-424, :483-484 via dolfinx.io.XDMFFile).
    dolfinx stores the heavy data in HDF5; h5py is not available here, so the same XDMF 3 layout
    (mesh grid + temporal collection of the nodal attribute "Temperature (K)") points at raw
    little-endian binary files instead (``Format="Binary"``, readable by ParaView/VisIt):
    ``output_xy.bin`` (n x 2 float64), ``output_conn.bin`` (n_e x 3 int32) and
    ``output_fields.f64`` (one field per step, initial state first, addressed with ``Seek``)."""

    def __init__(self, folder, coords, tris, tags):
        self.folder = folder
        self.n, self.ne = len(coords), len(tris)
        np.ascontiguousarray(coords, dtype="<f8").tofile(os.path.join(folder, "output_xy.bin"))
        np.ascontiguousarray(tris, dtype="<i4").tofile(os.path.join(folder, "output_conn.bin"))
        np.ascontiguousarray(tags, dtype="<i4").tofile(os.path.join(folder, "output_cell_tags.bin"))
        self.f = open(os.path.join(folder, "output_fields.f64"), "wb")
        self.times = []

    def __call__(self, t, u):
        np.asarray(u, dtype="<f8").tofile(self.f)
        self.times.append(float(t))

    def close(self):
        self.f.close()
        n, ne = self.n, self.ne
        item = 'Format="Binary" Endian="Little"'
        out = ['<?xml version="1.0"?>', '<Xdmf Version="3.0" xmlns:xi="http://www.w3.org/2001/XInclude">', " <Domain>",
               '  <Grid Name="mesh" GridType="Uniform">',
               f'   <Topology TopologyType="Triangle" NumberOfElements="{ne}" NodesPerElement="3">',
               f'    <DataItem {item} DataType="Int" Precision="4" Dimensions="{ne} 3">output_conn.bin</DataItem>',
               "   </Topology>", '   <Geometry GeometryType="XY">',
               f'    <DataItem {item} DataType="Float" Precision="8" Dimensions="{n} 2">output_xy.bin</DataItem>',
               "   </Geometry>", "  </Grid>",
               '  <Grid Name="Temperature (K)" GridType="Collection" CollectionType="Temporal">']
        for k, t in enumerate(self.times):
            out += ['   <Grid Name="Temperature (K)" GridType="Uniform">',
                    "    <xi:include xpointer=\"xpointer(/Xdmf/Domain/Grid[@GridType='Uniform'][1]/*[self::Topology or self::Geometry])\" />",
                    f'    <Time Value="{t!r}" />',
                    '    <Attribute Name="Temperature (K)" AttributeType="Scalar" Center="Node">',
                    f'     <DataItem {item} DataType="Float" Precision="8" Seek="{8 * n * k}" Dimensions="{n} 1">output_fields.f64</DataItem>',
                    "    </Attribute>", "   </Grid>"]
        out += ["  </Grid>", " </Domain>", "</Xdmf>"]
        with open(os.path.join(self.folder, "output.xdmf"), "w") as f:
            f.write("\n".join(out) + "\n")
        with open(os.path.join(self.folder, "output_fields.json"), "w") as f:
            json.dump({"name": "Temperature (K)", "n": n, "times": self.times, "dtype": "float64"}, f)


def run_simulation_impl(kind, cfg, mesh_folder, rebuild_mesh=False, visualize_mesh=False, output_folder=None,
                        watcher_points=None, write_xdmf=True, suppress_print=False, *, device_id=0, backend=None,
                        session=None, rtol=DEFAULT_RTOL, max_it=DEFAULT_MAX_IT, read_flux=True, precond=None,
                        two_sided=False, tangents=None, monitor_tangents=False, monitor_sigma=None):
    with suppress_output(suppress_print):
        program_start = time.time()
        check_config(cfg)   # k_aniso blocks, and none of them next to a table key, before any mesh or session is made
        stack = stack_with_diamond(cfg) if kind == "with_diamond" else stack_no_diamond(cfg)
        own_session = session is None
        if own_session:
            coords, tris, tags, tag_map = prepare_mesh(cfg, mesh_folder, rebuild_mesh, stack)
            session = SimulationSession(coords, tris, tags, tag_map, device_id=device_id, backend=backend, rtol=rtol,
                                        max_it=max_it, precond=1 if precond is None else precond)
        if visualize_mesh:
            print("visualize_mesh: the gmsh GUI is not part of this build; open mesh.msh in gmsh instead.")
        _parse_watchers(watcher_points)  # validate before any work, as the reference does at :431-439

        if output_folder is not None:
            save_folder = output_folder
            os.makedirs(save_folder, exist_ok=True)
            with open(os.path.join(save_folder, "used_config.yaml"), "w") as f:
                _dump_yaml(_with_scheme(cfg), f)
        else:
            save_folder = os.path.join(os.getcwd(), "sim_outputs", "refactor_test")
            os.makedirs(save_folder, exist_ok=True)

        sink = _FieldWriter(save_folder, session.coords, session.tris, session.tags) if write_xdmf else None
        try:
            if sink is not None:
                sink(0.0, np.full(len(session.coords), float(cfg["heating"]["ic_temp"])))
            result = session.run(cfg, stack, watcher_points, field_sink=sink, read_flux=read_flux and kind == "no_diamond",
                                 two_sided=two_sided, tangents=tangents,
                                 **({"monitor_tangents": monitor_tangents} if monitor_tangents else {}),
                                 **({"monitor_sigma": monitor_sigma} if monitor_sigma is not None else {}))
        finally:
            if sink is not None:
                sink.close()
            if own_session:
                session.close()

        if watcher_points is not None:
            write_watcher_csv(os.path.join(save_folder, "watcher_points.csv"), result["times"], result["watcher_names"],
                              result["watchers"])
        if result.get("monitors") is not None:
            write_monitors_csv(os.path.join(save_folder, "monitors.csv"), result["times"], result["monitors"])
        if result.get("monitor_uncertainty") is not None:
            write_uncertainty_csv(os.path.join(save_folder, "monitor_uncertainty.csv"), result["times"], result["monitors"],
                                  result["monitor_uncertainty"])
        if result.get("flux") is not None:
            result["flux"].write(save_folder)
            print(f"Saved raw gradient data at r=0 nodes to {os.path.join(save_folder, 'radial_gradient_raw.csv')}")
        total = time.time() - program_start
        n_steps = len(result["times"])
        print("\n--- Timing Summary ---")
        print(f"Total time: {total:.2f} s")
        print(f"Startup time: {total - result['loop_time']:.2f} s")
        print(f"Loop time: {result['loop_time']:.2f} s")
        print(f"Average time per step: {result['loop_time'] / max(n_steps, 1):.4f} s")
        print("----------------------\n")
        result["save_folder"] = save_folder
        result["total_time"] = total
        return result


def run_simulation_batch_impl(kind, cfgs, output_folders, watcher_points_list, session, suppress_print=True, read_flux=False):
    """``run_simulation`` for 2, 4, 8 or 16 configurations of one resident mesh at once (SimulationSession.run_batch):
    the same per-run artefacts (``used_config.yaml``, ``watcher_points.csv``, with ``read_flux`` also run_no_diamond's
    ``radial_gradient.csv`` / ``radial_gradient_raw.csv``) in each output folder, no XDMF.  The columns of a batch are
    sampled at the same nodes: all configurations must name the same watcher points (``ValueError`` otherwise - the
    points of a sweep group share their geometry and therefore do).  Returns the list of result dicts."""
    with suppress_output(suppress_print):
        t0 = time.time()
        for c in cfgs:
            check_config(c)
        stacks = [stack_with_diamond(c) if kind == "with_diamond" else stack_no_diamond(c) for c in cfgs]
        parsed = [_parse_watchers(wp) for wp in watcher_points_list]
        for names_j, coords_j in parsed[1:]:
            if names_j != parsed[0][0] or not np.array_equal(np.asarray(coords_j, dtype=float), np.asarray(parsed[0][1], dtype=float)):
                raise ValueError("run_simulation_batch_impl: the configurations of a batch must share their watcher points "
                                 "(one set of sample nodes serves every column)")
        for cfg, folder in zip(cfgs, output_folders):
            os.makedirs(folder, exist_ok=True)
            with open(os.path.join(folder, "used_config.yaml"), "w") as f:
                _dump_yaml(_with_scheme(cfg), f)
        results = session.run_batch(cfgs, stacks, watcher_points_list[0], read_flux=read_flux and kind == "no_diamond")
        for res, folder, wp in zip(results, output_folders, watcher_points_list):
            if wp is not None:
                write_watcher_csv(os.path.join(folder, "watcher_points.csv"), res["times"], res["watcher_names"], res["watchers"])
            if res.get("flux") is not None:
                res["flux"].write(folder)
            if res.get("monitors") is not None:
                write_monitors_csv(os.path.join(folder, "monitors.csv"), res["times"], res["monitors"])
            res["save_folder"] = folder
            res["total_time"] = (time.time() - t0) / len(cfgs)
        return results


def cli(kind, argv=None):
    """Command line of the drivers.  (The reference's own CLI cannot start: argparse is given
    ``type='dict'``, run_with_diamond.py:540; ``--watcher-points`` takes JSON here.)"""
    import argparse

    p = argparse.ArgumentParser(description="Heatflow simulation runner (MI355X)")
    p.add_argument("--config", type=str, default="simulation_template.yaml")
    p.add_argument("--mesh-folder", type=str, default="meshes")
    p.add_argument("--rebuild-mesh", action="store_true")
    p.add_argument("--visualize-mesh", action="store_true")
    p.add_argument("--output-folder", type=str)
    p.add_argument("--watcher-points", type=json.loads, help='JSON, e.g. {"pside": [z, r]}')
    p.add_argument("--write-xdmf", action="store_true")
    p.add_argument("--suppress-print", action="store_true")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--monitor-sigma", nargs="+", metavar="NAME=REL",
                   help="relative one-sigma of input parameters (the names tangents accept, e.g. p_sample.rho_c=0.15 fwhm=0.1, under "
                        "heating.source.tangents: true also source.power=0.05 source.fwhm=0.1): "
                        "writes monitor_uncertainty.csv, the first-order one-sigma band of every monitor field (needs a monitors block)")
    a = p.parse_args(argv)
    sigma = None
    if a.monitor_sigma:
        sigma = {}
        for item in a.monitor_sigma:
            name, eq, rel = item.rpartition("=")
            try:
                sigma[name] = float(rel)
            except ValueError:
                eq = ""
            if not eq or not name:
                p.error(f"--monitor-sigma: NAME=REL expected, got {item!r}")
    with open(a.config) as f:
        cfg = yaml.safe_load(f)
    run_simulation_impl(kind, cfg, a.mesh_folder, a.rebuild_mesh, a.visualize_mesh, a.output_folder, a.watcher_points,
                        a.write_xdmf, a.suppress_print, device_id=a.device, **({"monitor_sigma": sigma} if sigma else {}))
    return 0


if __name__ == "__main__":
    sys.exit(cli("with_diamond"))
