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

import collections
import contextlib
import copy
import csv
import dataclasses
import functools
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
from .aniso import (CAPACITY_KINDS, DIRECTIONAL_HINT, PARAM_KINDS, aniso_tables, capacity_scale, check_capacity_names, check_config,
                    classify_param, refuse_aniso, refuse_aniso_tables)
from .kappa_t import (capacity_form, check_capacity_form, check_sweep_tables, check_table_tangents, material_cv_table, picard_control,
                      refuse_enthalpy, material_table, picard_sweeps, refuse_tables,
                      refuse_tables_unless_swept, sweep_tables, table_keys, table_param,
                      table_tangents)
from .mesh import Mesh, load_mesh_arrays
from .stepping import assembled_step, refuse_variable_steps, timing_plan
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
    for key, table_of, values in (("kappa_tables", material_table, "k"), ("rhoc_tables", material_cv_table, "rho_cv")):
        tables = {}
        for name, mat in sorted((cfg.get("mats") or {}).items()):
            t = table_of(name, mat) if isinstance(mat, dict) else None
            if t is not None:
                tables[name] = {"T0": float(t[0]), "dT": float(t[1]), values: [float(v) for v in t[2]]}
        if tables:
            out["timing"]["picard_sweeps"] = picard_sweeps(cfg)
            out[key] = tables
    return out


def build_pattern_blob(coords, tris, tags, device_id=0):
    """The connectivity-derived tables of a mesh (CSR pattern, compressed column lists, row-gather assembly
    lists), built ONCE on this GPU and returned as a uint8 array: a sweep hands it to every solver session of
    every rank (``SimulationSession(..., pattern=blob)``), which then installs instead of rebuilding."""
    from .hip_backend import HeatflowHIP

    with HeatflowHIP(device_id) as be:
        be.set_mesh(coords, tris, tags)
        return be.export_pattern()


def _table_key(tables):
    return tuple((t, float(v[0]), float(v[1]), tuple(float(x) for x in v[2])) for t, v in sorted(tables.items()))


@dataclasses.dataclass(frozen=True, eq=False)
class ProblemSpec:
    """What a resident HeatProblem is made for, apart from the conductivities (which are re-valued in place): a session reuses its
    problem exactly while :attr:`key` stays the same, and makes one with :meth:`problem_kwargs`.  Both derive from the same
    fields, so a feature that adds a field is in the key as soon as it is in the keywords."""

    dt: float
    scheme: str
    rho_c: dict                         # {cell tag: rho cv}
    bcs: list                           # RowDirichletBC in application order
    kappa_tables: dict = dataclasses.field(default_factory=dict)      # {cell tag: (T0, dT, values)}
    rhoc_tables: dict = dataclasses.field(default_factory=dict)
    picard: int = 1                     # sweeps per step (the cap under the enthalpy form); it counts only with tables
    enthalpy: bool = False              # timing.capacity_form: enthalpy, with its tolerance and relaxation
    picard_tol: float | None = None
    picard_relax: float = 1.0
    k_aniso: dict = dataclasses.field(default_factory=dict)           # {cell tag: (m_r, m_z)}
    source: dict | None = None          # dict(tags, fwhm, z0, depth)
    monitors: dict | None = None        # {region: {"tags", "above"}}
    aniso_tables: bool = False          # timing.aniso_tables: the context's switch is set when the problem is made
    batch_tables: bool = False          # timing.sweep_tables: run_batch sets the context's switch on the problem it opens its batch on

    @property
    def tabled(self):
        return bool(self.kappa_tables or self.rhoc_tables)

    @functools.cached_property
    def key(self):
        """Hashable; the resident problem is reusable only for exactly the same Dirichlet DOF sets, in the same order, time step,
        capacities and scheme, and the same of every feature that is switched on.  Regions and source tags count in their given
        order; ``batch_tables`` is in the key and not in the keywords (the batch sets that switch itself)."""
        key = (self.dt, tuple(sorted(self.rho_c.items())),
               tuple(hashlib.sha1(np.ascontiguousarray(b.row_dofs, dtype=np.int64).tobytes()).hexdigest() for b in self.bcs),
               self.scheme)
        if self.tabled:
            key += (_table_key(self.kappa_tables), self.picard)
            if self.rhoc_tables:
                key += (_table_key(self.rhoc_tables),)
            if self.enthalpy:
                key += (("capacity_form", "enthalpy", self.picard_tol, self.picard_relax),)
        if self.k_aniso:
            key += (("k_aniso",) + tuple(sorted(self.k_aniso.items())),)
        if self.source:
            key += (("source", tuple(self.source["tags"]), self.source["fwhm"], self.source["z0"], self.source["depth"]),)
        if self.monitors:
            key += (("monitors",) + tuple((region, tuple(r["tags"]), r["above"]) for region, r in self.monitors.items()),)
        for name in ("aniso_tables", "batch_tables"):
            if getattr(self, name):
                key += ((name,),)
        return key

    def problem_kwargs(self):
        """HeatProblem's keywords after the positional (mesh, k, rho_c, dt, bcs, u0); a feature that is off adds none."""
        kw = {"scheme": self.scheme}
        if self.tabled:
            kw.update(kappa_tables=self.kappa_tables, picard=self.picard)
        if self.rhoc_tables:
            kw["rhoc_tables"] = self.rhoc_tables
        if self.enthalpy:
            kw.update(capacity_form="enthalpy", picard_tol=self.picard_tol, picard_relax=self.picard_relax)
        for name in ("k_aniso", "source", "monitors", "aniso_tables"):
            if getattr(self, name):
                kw[name] = getattr(self, name)
        return kw


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
        self._spec = None          # the ProblemSpec of the resident problem
        self._source_F1 = None     # the resident problem's source vector, read back once per problem
        self._source_G = None      # its derivatives (G_f, G_d), read back once per problem by the first tangent run under it
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
        self._ensure_problem(self.spec(cfg, stack), self._tables(stack)[0], float(cfg["heating"]["ic_temp"]))

    def spec(self, cfg, stack, two_sided=False, lagged_for=None):
        """The :class:`ProblemSpec` of ``cfg`` on this session's mesh; ValueError for what a forward run of it refuses.
        ``lagged_for`` names a request that runs the lagged capacity form only (tangents=): the enthalpy form is refused for it,
        before the form's own keys are checked."""
        shared = self._shared_spec(cfg, stack, two_sided)
        if lagged_for:
            refuse_enthalpy(cfg, lagged_for)
        return dataclasses.replace(shared, **self._table_fields(cfg, stack), source=self._source(cfg, stack),
                                   monitors=self._monitors(cfg), aniso_tables=aniso_tables(cfg))

    def _shared_spec(self, cfg, stack, two_sided=False):
        """The part of the spec the columns of a batch must share: time step, scheme, capacities, Dirichlet sets, anisotropy."""
        dt = assembled_step(cfg)     # t_final / num_steps; the first step under timing.steps, dt_init under timing.adaptive
        bcs = self._boundary_conditions(cfg, stack, two_sided)
        aniso = {self.material_tags[m.name]: m.properties["k_aniso"] for m in stack.materials if "k_aniso" in m.properties}
        return ProblemSpec(dt, time_scheme(cfg), self._tables(stack)[1], bcs, k_aniso=aniso)

    def _tables(self, stack):
        tag_to_k = {self.material_tags[m.name]: m.properties["k"] for m in stack.materials}
        tag_to_rc = {self.material_tags[m.name]: m.properties["rho_cv"] for m in stack.materials}
        return tag_to_k, tag_to_rc

    def _source(self, cfg, stack):
        """dict(tags, fwhm, z0, depth) of a configuration with a ``heating.source`` block (HeatProblem's ``source=``), or None."""
        spec = parse_source(cfg)
        return None if spec is None else spec.problem_source(stack, self.material_tags)

    def _monitors(self, cfg):
        """{region: {"tags", "above"}} of a configuration with a ``monitors`` block (HeatProblem's ``monitors=``), or None."""
        spec = parse_monitors(cfg)
        return None if spec is None else problem_monitors(spec, self.material_tags)

    def _table_fields(self, cfg, stack):
        """The spec's fields of a kappa(T) / cv(T) configuration: the tables {tag: (T0, dT, values)}, the Picard sweeps and, under
        timing.capacity_form: enthalpy, the form with its control; {} without tables."""
        tables = {self.material_tags[m.name]: m.properties["k_table"] for m in stack.materials if "k_table" in m.properties}
        ctables = {self.material_tags[m.name]: m.properties["rho_cv_table"] for m in stack.materials
                   if "rho_cv_table" in m.properties}
        form = check_capacity_form(cfg)
        if not (tables or ctables):
            return {}
        fields = {"kappa_tables": tables, "rhoc_tables": ctables, "picard": picard_sweeps(cfg)}
        if form == "enthalpy":     # (absent / lagged: HeatProblem sees the arguments of before)
            tol, relax = picard_control(cfg)
            fields.update(enthalpy=True, picard_tol=tol, picard_relax=relax)
        return fields

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

    def _ensure_problem(self, spec, tag_to_k, ic_temp):
        """The resident HeatProblem for ``spec`` (built if absent), its operator valued for ``tag_to_k``.  True if it was built."""
        if self.problem is None or spec.key != self._spec.key:
            self.close()
            print("Assigning material properties...")
            shared = self.hierarchy if (self.hierarchy is not None and self.precond == 1) else None
            self.problem = HeatProblem(self.coords, self.tris, self.tags, tag_to_k, spec.rho_c, spec.dt, spec.bcs, ic_temp,
                                       backend=self.backend, device_id=self.device_id, rtol=self.rtol,
                                       max_it=self.max_it, assembly_mode=self.assembly_mode, precond=self.precond,
                                       amg_reuse=True, pattern=self.pattern, amg=shared["blob"] if shared else None,
                                       **spec.problem_kwargs())
            self._spec = spec
            self._source_F1 = None
            self._source_G = None
            self._k = dict(tag_to_k)
            # conductivities the multigrid levels were built for: this problem's, or those of the session that shared them
            self._k_hier = dict(shared["k"]) if shared else dict(tag_to_k)
            self.hierarchy = None                    # a later problem of this session (other dt / Dirichlet set) builds its own
            if shared and set(self._k_hier) == set(tag_to_k) and self._out_of_range(tag_to_k):
                self._rebuild_hierarchy(tag_to_k)    # too far from this point's operator to be a good frozen hierarchy
            print("Material properties assigned.")
            return True
        self.problem.bcs = spec.bcs
        if tag_to_k != self._k:
            self._revalue(tag_to_k)
        return False

    def _out_of_range(self, *k_maps):
        """The frozen coarse levels stay a good preconditioner while no conductivity moved by more than 2x from the values they
        were built for (measured: 3.8 -> 60 W/m/K triples the iteration count): True if one of ``k_maps`` is beyond that."""
        return max(max(k[t] / self._k_hier[t], self._k_hier[t] / k[t]) for k in k_maps for t in k) > 2.0

    def _rebuild_hierarchy(self, tag_to_k):
        """Re-value the resident operator for ``tag_to_k`` and build the multigrid levels from it."""
        be = self.problem.backend
        be.set_precond(1, False)
        self.problem.set_materials(tag_to_k, self._spec.rho_c)
        be.set_precond(1, True)
        self._k_hier = dict(tag_to_k)

    def _revalue(self, tag_to_k, allow_rebuild=True):
        # re-value A on the resident pattern, and beyond the hierarchy's range rebuild it
        if self._out_of_range(tag_to_k) and self.precond == 1 and allow_rebuild:
            self._rebuild_hierarchy(tag_to_k)
        else:
            self.problem.set_materials(tag_to_k, self._spec.rho_c)
        self._k = dict(tag_to_k)

    def _watcher_nodes(self, watcher_points):
        names, coords_w = _parse_watchers(watcher_points)
        if not names:
            return names, None
        from .solver import nearest_nodes
        return names, nearest_nodes(self.coords, coords_w)

    def _flux_sampler(self, read_flux):
        """A FluxSampler of this mesh with ``read_flux`` (else None), the resident problem's projection set up."""
        if not read_flux:
            return None
        if not getattr(self.problem, "_flux_ready", False):
            print("Setting up radial heat flux sampling...")
            self.problem.backend.flux_setup()  # once per mesh: the unit-coefficient mass matrix does not depend on kappa
            self.problem._flux_ready = True
        return FluxSampler(self.coords)

    def _check_batch(self, cfgs, stacks):
        """What the configurations of a batch must not ask for and must share, apart from the problem's own spec; a mismatch is a
        ValueError naming what differs.  Returns (their parsed sources, the absorbing face's z or None, the problem's monitors,
        whether any of them carries tables)."""
        for c in cfgs:
            refuse_enthalpy(c, "run_batch (the batched loop)")
            refuse_variable_steps(c, "run_batch (the batched loop)")
            check_sweep_tables(c, "run_batch (the batched loop)")
            refuse_tables_unless_swept(c, "run_batch (the batched loop)")
            refuse_source_sweeps(c, "run_batch (the batched loop)")
            refuse_monitors_sweeps(c, "run_batch (the batched loop)")
        if len(cfgs) not in (2, 4, 8, 16):
            raise ValueError("run_batch: 2, 4, 8 or 16 configurations at a time")
        specs, z0 = [parse_source(c) for c in cfgs], None
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
            z0 = z0s[0]
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
        return specs, z0, mon, any(tabled)

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
        sources, z0, mon, tabled = self._check_batch(cfgs, stacks)
        t_start = time.time()
        num_steps = int(cfgs[0]["timing"]["num_steps"])
        ic_temp = float(cfgs[0]["heating"]["ic_temp"])
        cols = []                # (what the columns must share, conductivities) per column
        for cfg, stack in zip(cfgs, stacks):
            cols.append((self._shared_spec(cfg, stack), self._tables(stack)[0]))
            if int(cfg["timing"]["num_steps"]) != num_steps or float(cfg["heating"]["ic_temp"]) != ic_temp \
                    or cols[-1][0].key != cols[0][0].key:
                raise ValueError("run_batch: the configurations must share time stepping (and scheme), ic_temp, rho_c, the Dirichlet sets "
                                 "and the anisotropy multipliers (k_aniso)")
        percol = any(tk != cols[0][1] for _, tk in cols)
        mid, mid_k = cols[nv // 2]
        # conductivities that differ between the columns; a single one (sweep_test.py's kappa_sample list) makes
        # the operators an affine family A + (kappa_j - kappa_ref) A1: two shared matrices instead of nv
        varying = [t for t in mid_k if any(tk[t] != mid_k[t] for _, tk in cols)]
        affine = percol and len(varying) == 1
        # the batch's problem carries the monitors' table and no source of its own (the batch gets one: hf_batch_begin refuses the
        # context's); under tables every column has its own operator, re-valued by the batch itself
        fields = self._table_fields(cfgs[nv // 2], stacks[nv // 2]) if tabled else {}
        spec = dataclasses.replace(mid, monitors=mon, batch_tables=bool(fields), **fields)
        if spec.tabled:
            percol, affine = True, False
        # a resident problem that differs by its source alone (a single run before, or prepare) gives the source up
        if sources[0] is not None and self.problem is not None and self.problem.source and \
                self._spec.key == dataclasses.replace(spec, source=self.problem.source).key:
            self.problem.backend.set_source(None)
            self.problem.source = None
            self._spec, self._source_F1, self._source_G = spec, None, None
        self._ensure_problem(spec, mid_k, ic_temp)
        prob = self.problem
        be = prob.backend
        # all columns share the hierarchy: keep every column within its range
        if percol and self.precond == 1 and self._out_of_range(*(tk for _, tk in cols)):
            self._rebuild_hierarchy(mid_k)
            self._k = dict(mid_k)
        times = (np.arange(num_steps) + 1) * spec.dt
        g_all = np.empty((num_steps, len(prob.bc_dofs), nv), dtype=np.float64)
        tabulated = {}                                   # columns with the same boundary definition share one table
        for j, (col, _) in enumerate(cols):
            bcs, h = col.bcs, cfgs[j]["heating"]
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
        prob.bcs = cols[-1][0].bcs
        names, nodes = self._watcher_nodes(watcher_points)
        if affine and mid_k != self._k:
            self._revalue(mid_k, allow_rebuild=False)     # the context's operator is the reference of the family
        flux0 = self._flux_sampler(read_flux)
        if spec.tabled:
            be.set_state(np.full(prob.n, ic_temp))       # (a resident problem may stand at the end of an earlier run)
            be.set_batch_tables(True)
        be.batch_begin(nv, per_column_operator=2 if affine else (1 if percol else 0))
        try:
            if spec.tabled:      # the constants of the materials without a conductivity table, column by column
                free = sorted(t for t in mid_k if t not in spec.kappa_tables)
                for j, (_, tk) in enumerate(cols):
                    be.batch_set_column_kappa(j, free, [tk[t] for t in free])
            elif affine:
                be.batch_set_affine(varying, [tk[varying[0]] - mid_k[varying[0]] for _, tk in cols])
            elif percol:
                for j, (_, tk) in enumerate(cols):
                    if tk != self._k:
                        self._revalue(tk, allow_rebuild=False)
                    be.batch_load_column(j)
            for j in range(nv):
                be.batch_set_state(j, np.full(prob.n, ic_temp))
            if sources[0] is not None:   # the batch's own source; W -> W/m^3 per step and column, from each column's own integral
                be.batch_set_source([int(self.material_tags[m]) for m in sources[0].materials], [sp.fwhm for sp in sources], z0,
                                    [sp.depth for sp in sources])
                amp, vectors = np.empty((num_steps, nv), dtype=np.float64), {}
                for j, sp in enumerate(sources):
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
                 "n_dof": prob.n, "dt": spec.dt, "flux": fluxes[j], "batch": nv,
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
        tangents, monitor_tangents, sigma, source = self._check_request(cfg, tangents, monitor_tangents, monitor_sigma)
        arg = "monitor_sigma" if monitor_sigma is not None else "tangents"
        # the time loop's plan (heatflow_amd.stepping.timing_plan): equal steps, a list, or controlled steps
        plan, plan_data = timing_plan(cfg)
        if plan != "uniform":
            if tangents:
                refuse_variable_steps(cfg, arg + "=")
            if read_flux:
                refuse_variable_steps(cfg, "the read-flux run")
            if capacity_form(cfg) == "enthalpy":
                refuse_variable_steps(cfg, "timing.capacity_form: enthalpy")
        dts = np.asarray(plan_data, dtype=np.float64) if plan == "steps" else None
        num_steps = plan_data if plan == "uniform" else len(dts) if plan == "steps" else 0
        ic_temp = float(cfg["heating"]["ic_temp"])
        spec = self.spec(cfg, stack, two_sided, lagged_for=arg + "=" if tangents else None)
        tab_on = bool(tangents) and self._check_tangent_request(cfg, spec, tangents, monitor_tangents, arg)
        dt, varying, mon = spec.dt, spec.bcs[3:], spec.monitors
        fresh = self._ensure_problem(spec, self._tables(stack)[0], ic_temp)
        if not fresh:
            self.problem.set_state(ic_temp)
            self.problem.iters = []
        prob = self.problem
        if mon and not fresh:    # the records of this run only
            prob.clear_monitor_history()
        if spec.enthalpy:        # the sweeps and changes of this run only; with monitors the stored heat per step, for `energy`
            if not fresh:
                prob.clear_picard_history()
            if mon:
                prob.clear_heat_history()
                prob.record_heat()
        amp = None
        if source is not None:   # W -> W/m^3 per step, from the discrete source's own integral
            if self._source_F1 is None:
                self._source_F1 = prob.source_vector()
            if plan == "adaptive":   # the step ends are not known beforehand: the amplitude of any time
                F1 = self._source_F1
                amp = lambda t: float(source_amplitudes(source, np.array([float(t)]), F1, _resolve)[0])
            else:
                ends = np.cumsum(dts) if plan == "steps" else (np.arange(num_steps) + 1) * dt
                amp = source_amplitudes(source, ends, self._source_F1, _resolve)
        names, nodes = self._watcher_nodes(watcher_points)

        flux = self._flux_sampler(read_flux)
        print("Beginning loop...")
        t_loop = time.time()
        tangent_out, extra = {}, {}
        if tangents:
            if field_sink is not None or flux is not None:
                raise ValueError("tangents: not combined with a field sink or the read-flux projection")
            cols = self._tangent_columns(cfg, source, list(tangents), tab_on, monitor_tangents, (np.arange(num_steps) + 1) * dt, amp)
            times, samples, tsamp, iters, titers = prob.run_tangent(num_steps, nodes, time_varying=varying, **cols.kwargs)
            tangent_out, extra = self._tangent_results(cfg, list(tangents), names, tsamp, titers, cols.scale, monitor_tangents, sigma)
        elif plan == "adaptive":
            sink = None if field_sink is None else (lambda t: field_sink(t, prob.state()))
            times, samples, iters, info = prob.run_adaptive(float(cfg["timing"]["t_final"]), plan_data["tol"], watcher_nodes=nodes,
                                                            time_varying=varying, on_accept=sink,
                                                            **{k: v for k, v in plan_data.items() if k != "tol"},
                                                            **({"source_amplitude": amp} if amp is not None else {}))
            extra = {"steps_taken": [float(h) for h in info["dt"]],
                     "adaptive": {k: info[k] for k in ("accepted", "rejected", "revaluations")}}
            num_steps = len(times)
        elif plan == "steps" and field_sink is None:
            times, samples, iters = prob.run_steps(dts, watcher_nodes=nodes, time_varying=varying,
                                                   **({"source_amplitude": amp} if amp is not None else {}))
        elif field_sink is None and flux is None:
            times, samples, iters = prob.run(num_steps, watcher_nodes=nodes, time_varying=varying,
                                             **({"source_amplitude": amp} if amp is not None else {}))
        else:  # step-wise: every field goes to the sink (visualisation) and / or through the flux projection
            times, samples, iters = self._run_stepwise(spec.bcs, num_steps, dt, amp, nodes, flux, field_sink, dts)
        loop_time = time.time() - t_loop
        print(f"Simulation progress: 100% (step {num_steps}/{num_steps}) | Avg time/step: {loop_time / num_steps:.4f} s"
              f" | PCG iterations/step: mean {np.mean(iters):.0f}, max {int(np.max(iters))}")
        return {
            "times": np.asarray(times), "watcher_names": names,
            "watchers": {nm: samples[:, k] for k, nm in enumerate(names)},
            "iters": np.asarray(iters), "loop_time": loop_time, "startup_time": t_loop - t_start,
            "n_dof": prob.n, "dt": dt, "flux": flux,
            **tangent_out,
            **self._history_results(spec),
            **extra,
        }

    # -- the steps of run(), each in the order run() takes them --------------------------------------------------------------------
    def _check_request(self, cfg, tangents, monitor_tangents, monitor_sigma):
        """What a run is asked for against the configuration alone, before any problem is made: (the tangent columns with those
        ``monitor_sigma`` implies, whether the monitors' derivatives are wanted, the checked sigmas or None, the parsed source
        or None); ValueError naming the argument or the parameter otherwise."""
        sigma = None
        if monitor_tangents or monitor_sigma is not None:
            arg = "monitor_sigma" if monitor_sigma is not None else "monitor_tangents"
            if parse_monitors(cfg) is None:
                raise ValueError(f"{arg}: the configuration has no monitors block (heatflow_amd.monitors)")
            sigma = check_sigma(monitor_sigma) if monitor_sigma is not None else None
            tangents = list(tangents or ()) + [q for q in sigma or () if q not in (tangents or ())]
            if not tangents:
                raise ValueError("monitor_tangents: no parameter (tangents= names the columns)")
            if len(tangents) > 16:
                raise ValueError(f"{arg}: {len(tangents)} tangent columns (at most 16 per run)")
            monitor_tangents = True
        spec = parse_source(cfg)
        if spec is not None and tangents and not spec.tangents:
            refuse_source(cfg, "tangents=")
        for p in tangents or ():     # the source's own names, and the names a source rules out
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
        return tangents, monitor_tangents, sigma, spec

    def _check_tangent_request(self, cfg, spec, tangents, monitor_tangents, arg):
        """What tangent columns rule out in the problem ``spec`` describes, before it is made.  Returns whether the run
        differentiates through the tables (timing.table_tangents)."""
        refuse_aniso_tables(cfg, arg)    # both kinds: timing.aniso_tables covers the forward run only, with timing.table_tangents too
        tab_on = spec.tabled and table_tangents(cfg)
        if spec.tabled and not tab_on:
            refuse_tables(cfg, "tangents")
        if tab_on:
            if monitor_tangents:
                raise ValueError(("monitor_sigma" if arg == "monitor_sigma" else "monitor_tangents")
                                 + ": monitor derivatives together with timing.table_tangents are not supported")
            check_table_tangents(cfg, "tangents", tangents)
            for p in tangents:       # the names of the tables' parameters
                try:
                    tp = None if p == "fwhm" else table_param(cfg, p)
                except ValueError as e:
                    raise ValueError(f"tangents: {e}") from None
                mat, _, suffix = p.rpartition(".")
                if tp is None and suffix in ("k_r", "k_z") and self.material_tags.get(mat) in spec.kappa_tables:
                    raise ValueError(f"tangents: parameter {p!r}: {mat!r} carries a conductivity table (its parameters are "
                                     f"{mat}.k or {mat}.k_power.exponent, or {mat}.k_table.scale)")
        if spec.k_aniso:         # a bare name means the isotropic k: an anisotropic material is named by direction
            refuse_aniso(cfg, "a tangent with respect to the conductivity of an anisotropic material", set(tangents),
                         DIRECTIONAL_HINT)
        return tab_on

    def _tangent_columns(self, cfg, source, params, tab_on, monitor_tangents, times, amp):
        """The columns of ``params`` as HeatProblem.run_tangent takes them: TangentColumns(its keywords, {column: the factor
        that turns the column's rho_c tangent into the named capacity parameter's})."""
        prob = self.problem
        try:
            check_capacity_names(params)
        except ValueError as e:
            raise ValueError(f"tangents: {e}") from None
        cond, bnd, shp, cap, cscale, srcp, tabs = [], {}, {}, {}, {}, {}, {}
        for j, p in enumerate(params):
            try:
                kind, mat = classify_param(p, tables=tab_on)
                tp = table_param(cfg, p) if tab_on and kind != "fwhm" else None
                if kind == "thickness" and mat in self.material_tags:
                    check_thickness_name(cfg, mat, p)
            except ValueError as e:
                raise ValueError(f"tangents: {e}") from None
            cond.append([])
            if tp is not None:       # a parameter of a material's table: a derivative table on the table's own grid
                tabs[j] = {tp[1]: {self.material_tags[tp[0]]: tp[2]}}
            elif kind == "source":
                srcp[j] = p
            elif kind == "fwhm":
                bnd[j] = {3 + q: h.gaussian_dfwhm for q, h in enumerate(self._heats)}
                if source is not None and "fwhm" not in source_block(cfg):     # the beam takes heating.fwhm too: both terms
                    srcp[j] = "source.fwhm"
            elif mat not in self.material_tags:
                raise ValueError(f"tangents: unknown parameter {p!r} (a material name, <material>.k_r, "
                                 "<material>.k_z, <material>.k, <material>.thickness or 'fwhm')")
            elif kind == "thickness":     # the nodes of this session's mesh move with the stack of ``cfg``
                shp[j] = thickness_velocity(cfg, mat, self.coords[:, 0])
            elif kind in CAPACITY_KINDS:  # a column in rho_c = rho cv of the material; cv and rho by the chain rule
                if mat not in (cfg.get("mats") or {}):
                    raise ValueError(f"tangents: parameter {p!r}: no material {mat!r} in the configuration")
                cap[j] = [self.material_tags[mat]]
                cscale[j] = capacity_scale(cfg["mats"][mat], CAPACITY_KINDS[kind])
            else:                         # the bare name: the set-up of isotropic tags; "<m>.k" / ".k_r" / ".k_z": the directional one
                cond[j] = [self.material_tags[mat] if p == mat else (self.material_tags[mat], PARAM_KINDS[kind])]
        kwargs = {"conductivity": cond, "boundary": bnd, **({"shape": shp} if shp else {}),
                  **({"capacity": [cap.get(j, []) for j in range(len(params))]} if cap else {}),
                  **({"monitor_tangents": True} if monitor_tangents else {}), **({"tables": tabs} if tab_on else {})}
        if source is not None:   # the opt-in: the source becomes differentiable, its own parameters get their columns
            src_cols = {}
            if srcp:
                if self._source_G is None:
                    self._source_G = (prob.source_derivative("fwhm"), prob.source_derivative("depth"))
                table = tangent_coefficients(source, sorted(set(srcp.values())), times, self._source_F1, self._source_G[0],
                                             self._source_G[1], _resolve)
                src_cols = {j: {"amplitude": table[p][:, 0], "fwhm": table[p][:, 1], "depth": table[p][:, 2]}
                            for j, p in srcp.items()}
            kwargs.update(source=src_cols, source_amplitude=amp)
        return TangentColumns(kwargs, cscale)

    def _tangent_results(self, cfg, params, names, tsamp, titers, cscale, monitor_tangents, sigma):
        """The result entries of a tangent run, in two parts: ``tangents`` and ``tangent_iters``; with the monitors' derivatives
        ``monitor_tangents`` and (under ``monitor_sigma``, ``sigma`` not None) ``monitor_uncertainty``."""
        for j, f in cscale.items():
            if f != 1.0:
                tsamp[:, j] *= f
        out = {"tangents": {p: {nm: tsamp[:, j, k] for k, nm in enumerate(names)} for j, p in enumerate(params)},
               "tangent_iters": titers}
        extra = {}
        if monitor_tangents:
            dhist = self.problem.monitor_tangent_history(scale=[cscale.get(j, 1.0) for j in range(len(params))])
            extra["monitor_tangents"] = {p: {region: {field: d[:, j] for field, d in f.items()} for region, f in dhist.items()}
                                         for j, p in enumerate(params)}
            if sigma is not None:
                from .fit import get_param
                extra["monitor_uncertainty"] = monitor_uncertainty(extra["monitor_tangents"],
                                                                   {q: s * get_param(cfg, q) for q, s in sigma.items()})
        return out, extra

    def _run_stepwise(self, bcs, num_steps, dt, amp, nodes, flux, field_sink, dts=None):
        """The steps one by one: every field goes to ``field_sink`` and / or through the flux projection of ``flux``.  ``dts``: the
        sizes of a step list (timing.steps); None: equal steps of ``dt``."""
        prob = self.problem
        for bc in bcs:
            bc.update(0.0)
        times, rows, iters = [], [], []
        ends = None if dts is None else np.cumsum(dts)
        try:
            return self._stepwise_loop(prob, bcs, num_steps, dt, amp, nodes, flux, field_sink, dts, ends, times, rows, iters)
        finally:
            if dts is not None:
                prob._restore_step()

    def _stepwise_loop(self, prob, bcs, num_steps, dt, amp, nodes, flux, field_sink, dts, ends, times, rows, iters):
        for step in range(num_steps):
            t = (step + 1) * dt if dts is None else float(ends[step])
            if dts is not None:
                prob.backend.set_step(float(dts[step]))
            it, _ = prob.step(t, only=bcs[3:], **({"source_amplitude": float(amp[step])} if amp is not None else {}))
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
        return np.array(times), np.array(rows), np.array(iters)

    def _history_results(self, spec):
        """The result entries the resident problem recorded along the run: ``monitors`` and, under the enthalpy form, ``picard``
        (with a RuntimeWarning for steps that ended at the sweep cap above the tolerance)."""
        prob, out = self.problem, {}
        if spec.monitors:
            out["monitors"] = prob.monitor_history()
            if spec.enthalpy:    # every region's energy from the heat records: the stored heat the scheme conserves, tabled tags included
                heat = prob.heat_history()
                for region, r in spec.monitors.items():
                    out["monitors"][region]["energy"] = sum(heat[int(t)] for t in r["tags"])
        if spec.enthalpy:
            hist = prob.picard_history()
            sweeps, change = np.asarray(hist["sweeps"]), np.asarray(hist["change"])
            out["picard"] = {"sweeps": sweeps, "change": change}
            if spec.picard_tol:
                late = np.flatnonzero((sweeps >= spec.picard) & (change > spec.picard_tol))
                if late.size:
                    warnings.warn(f"timing.picard_sweeps = {spec.picard}: step {int(late[0]) + 1} ended at the cap with a Picard "
                                  f"change of {change[late[0]]:.3g} K > timing.picard_tol = {spec.picard_tol:g} K "
                                  f"({late.size} such step(s); more sweeps or timing.picard_relax < 1 may help)", RuntimeWarning,
                                  stacklevel=3)
        return out


TangentColumns = collections.namedtuple("TangentColumns", "kwargs scale")


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

        if result.get("steps_taken") is not None and output_folder is not None:
            # an adaptive run: the accepted step sizes, so that the run can be replayed as a list (HeatProblem.run_steps)
            used = _with_scheme(cfg)
            used["timing"] = dict(used["timing"], steps_taken=[float(h) for h in result["steps_taken"]])
            with open(os.path.join(save_folder, "used_config.yaml"), "w") as f:
                _dump_yaml(used, f)
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
