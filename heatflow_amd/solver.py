"""Backward-Euler (or, opt-in, BDF2) heat problem on the HIP backend.

Host-side equivalent of the block *forms -> assemble_matrix -> KSP -> time loop* of the
reference drivers (run_with_diamond.py:321-394, 456-504), with the seven dolfinx/PETSc
calls replaced by libheatflow_hip.so (see include/heatflow_hip.h for the mapping).

The loop order is the reference's: ``bc.update(t)`` -> RHS (M u^n, lifting, set_bc) ->
solve in place -> sample watchers.  The solver differs by design: Jacobi-PCG on the
GPU instead of a cached MUMPS LU; it stops at ``||D^-1 r|| <= rtol ||D^-1 b||``
(Kelvin-scaled residual) and reports the iteration count of every step.
"""
from __future__ import annotations

import hashlib
import time

import numpy as np

from .bc import gather_bc_values, gather_plan, merge_bcs
from .hip_backend import ASM_ROW_GATHER, PC_AMG, PC_JACOBI, HeatflowHIP, time_scheme_code
from .monitors import check_regions, combine as combine_monitors, combine_tangents, tag_thresholds

# Default PCG tolerance: at rtol = 1e-10 the temperature field agrees with a sparse
# direct solve of the same system to ~3e-6 K (measured on the stock and the 1M-DOF
# meshes, tests/test_gpu_parity.py); the stated parity bound is 1e-4 K absolute.
DEFAULT_RTOL = 1e-10
DEFAULT_MAX_IT = 20000


class HeatProblem:
    """Mesh + coefficients + Dirichlet rows on one GPU context.

    Parameters
    ----------
    coords (n,2) [z,r], tris (n_e,3), tags (n_e,)
    tag_to_k, tag_to_rho_cv : {cell tag: value}   (run_with_diamond.py:286-287)
    dt : time step
    bcs : list of RowDirichletBC in application order (later wins on shared DOFs)
    u0 : scalar or (n,) initial temperature
    backend : an object with the HeatflowHIP interface; default = a new HeatflowHIP
    assembly_mode : ASM_ROW_GATHER (default: a lane per CSR row, no atomics, bitwise reproducible matrices),
              ASM_LDS_COLORED (LDS scatter by colours, reproducible), ASM_LDS_ATOMIC (LDS atomics, diagonals
              summed in arrival order) or ASM_GLOBAL_ATOMIC (baseline)
    pattern : connectivity tables exported by another context on the same mesh (HeatflowHIP.export_pattern)
    amg : multigrid hierarchy exported by another context on the same mesh (HeatflowHIP.amg_export; needs precond=PC_AMG
              and amg_reuse=True): installed instead of being built
    precond : PC_JACOBI (Jacobi-PCG, the north-star solver) or PC_AMG (PCG preconditioned by a
              smoothed-aggregation V-cycle: same stopping rule and answer, ~50x fewer iterations)
    scheme : "backward_euler" (default, the reference's scheme) or "bdf2" (second order, hf_set_time_scheme); ``dt`` stays
              the time step and the sample times stay (k+1) dt
    kappa_tables : {cell tag: (T0, dT, values)} - temperature-dependent conductivities (hf_set_kappa_tables):
              every step re-values the operator at u^n (BDF2: 2 u^n - u^{n-1}); the state u0 is set before the assembly, so
              the multigrid hierarchy is built from A(u0).  None / {}: constant conductivities, the call sequence of before.
    rhoc_tables : {cell tag: (T0, dT, values of rho * cv)} - temperature-dependent heat capacities (hf_set_rhoc_tables, DESIGN.md
              3.10): every evaluation re-values M as well as A.  With or without kappa_tables; the same order (tables, state,
              assembly).  None / {}: constant capacities.
    picard : Picard sweeps per step with tables (1..8; 1 = the lagged scheme); under ``capacity_form="enthalpy"`` the sweep cap
              (1..64)
    capacity_form : "lagged" (default: rho_c at the element temperature of the last iterate; no extra call is
              made) or "enthalpy" (hf_set_capacity_form): the chord capacity between u^n and the evaluation
              state, so that a converged step conserves the stored heat of :meth:`stored_heat`.  Needs ``rhoc_tables``;
              backward Euler only; not with ``k_aniso``; :meth:`run_tangent` and the batched sweeps are refused by the library.
    picard_tol : enthalpy form: stop a step's sweeps at max |x_k - e_{k-1}| <= picard_tol (K); None / 0: all ``picard`` sweeps
    picard_relax : enthalpy form: e_k = e_{k-1} + picard_relax (x_k - e_{k-1}), in (0, 1]
    k_aniso : {cell tag: (m_r, m_z)} - anisotropic conductivities (hf_set_anisotropy): the tag conducts with
              k_r = m_r k along r and k_z = m_z k along z.  Set right after the materials, before the first assembly.  Not
              together with kappa_tables / rhoc_tables (ValueError) unless ``aniso_tables``.  None / {}: isotropic, the call
              sequence of before.
    aniso_tables : True allows k_aniso together with kappa_tables / rhoc_tables (hf_set_aniso_tables): the switch
              is set right after the materials, before set_anisotropy and the tables; k_r = m_r kappa(T_e), k_z = m_z kappa(T_e).
              Forward runs and :meth:`solve_steady`; tangent runs of such a problem stay refused by the library.  False (default):
              the combination is a ValueError and no extra call is made.
    source : dict(tags=, fwhm=, z0=, depth=) - a volumetric source (hf_set_source): power absorbed in the cell
              tags ``tags`` with the shape exp(-4 ln2 r^2 / fwhm^2) exp(-|z - z0| / depth) (``depth`` absent or inf: uniform
              in z).  Set right after the materials; its amplitude per step is :meth:`run`'s ``source_amplitude``.  None: no
              source, the call sequence of before.
    monitors : {region: {"tags": [cell tags], "above": theta | None}} - region monitors (hf_set_monitors): after
              every step of :meth:`step`, :meth:`run` and :meth:`run_tangent` the GPU records, per tag, the extremes, the volume
              integrals and the part above ``above``; :meth:`monitor_history` and :meth:`monitors_now` combine them per region.
              Set right after the materials.  ``energy`` is measured from ``u0`` when it is a scalar (attribute
              ``monitor_T_ref``).  None / {}: no monitors, the call sequence of before.
    """

    def __init__(self, coords, tris, tags, tag_to_k, tag_to_rho_cv, dt, bcs, u0, *, backend=None, device_id=0,
                 assembly_mode=ASM_ROW_GATHER, rtol=DEFAULT_RTOL, atol=0.0, max_it=DEFAULT_MAX_IT,
                 precond=PC_JACOBI, amg_reuse=False, pattern=None, amg=None, scheme="backward_euler", kappa_tables=None,
                 picard=1, rhoc_tables=None, k_aniso=None, source=None, monitors=None, aniso_tables=False,
                 capacity_form="lagged", picard_tol=None, picard_relax=1.0):
        self.coords = np.ascontiguousarray(coords, dtype=np.float64)
        self.n = self.coords.shape[0]
        self.dt = float(dt)
        self.bcs = list(bcs)
        self.rtol, self.atol, self.max_it = float(rtol), float(atol), int(max_it)
        self.assembly_mode = assembly_mode
        self.precond = precond
        self.scheme = scheme
        self.kappa_tables = dict(kappa_tables or {})
        self.rhoc_tables = dict(rhoc_tables or {})
        self.picard = int(picard)
        self.k_aniso = check_k_aniso(k_aniso)
        self.aniso_tables = bool(aniso_tables)
        if self.k_aniso and (self.kappa_tables or self.rhoc_tables) and not self.aniso_tables:
            raise ValueError("HeatProblem: k_aniso together with kappa_tables / rhoc_tables is not supported "
                             "(the table kernels are isotropic)")
        self.capacity_form, self.picard_tol, self.picard_relax = check_capacity_form(
            capacity_form, self.picard, picard_tol, picard_relax, scheme=scheme, rhoc_tables=self.rhoc_tables, k_aniso=self.k_aniso)
        self.source = check_source(source)
        # hf_source_derivatives has been called for the source (run_tangent's source=, source_derivative).  False is always safe:
        # the call is made again.  Code that sets the source on the backend directly leaves the library refusing, whatever this says.
        self._source_diff = False
        self.monitors = check_regions(monitors)
        self._monitor_tags = tag_thresholds(self.monitors) if self.monitors else {}
        self.monitor_T_ref = float(u0) if np.isscalar(u0) else None
        scheme_code = time_scheme_code(scheme)     # (an unknown name raises before any backend call)
        self.backend = backend if backend is not None else HeatflowHIP(device_id)
        self._own_backend = backend is None

        t0 = time.perf_counter()
        if pattern is None:
            self.backend.set_mesh(self.coords, tris, tags)
        else:   # connectivity tables built once elsewhere (another rank / context of the sweep): install, do not rebuild
            self.backend.set_mesh(self.coords, tris, tags, pattern=pattern)
        self.mesh_seconds = time.perf_counter() - t0
        self.set_materials(tag_to_k, tag_to_rho_cv, assemble=False)
        if self.aniso_tables:    # (off is every context's default: no extra call)
            self.backend.set_aniso_tables(True)
        if self.k_aniso:         # isotropic problems make no extra call
            self.backend.set_anisotropy(self.k_aniso)
        if self.source:          # problems without a source make no extra call
            self.backend.set_source(self.source["tags"], self.source["fwhm"], self.source["z0"], self.source["depth"])
        if self.monitors:        # problems without monitors make no extra call
            self.backend.set_monitors(self._monitor_tags)
        if self.bcs:
            self.bc_dofs, self._owner, self._pos = merge_bcs(self.bcs)
        else:
            self.bc_dofs = np.zeros(0, dtype=np.int32)
            self._owner = self._pos = np.zeros(0, dtype=np.int64)
        self.backend.set_dirichlet(self.bc_dofs)
        self.backend.set_precond(precond, amg_reuse)
        if scheme_code != 0:     # backward Euler is every context's default: its path makes no extra call
            self.backend.set_time_scheme(scheme_code)
        if amg is not None and precond == PC_AMG and amg_reuse:
            self.backend.amg_install(amg)
        u = np.full(self.n, float(u0)) if np.isscalar(u0) else np.asarray(u0, dtype=np.float64)
        if self.kappa_tables or self.rhoc_tables:   # tables: the operator (and the hierarchy built from it) is evaluated at u0
            if self.kappa_tables:
                # (under the enthalpy form the cap, which may exceed this call's 1..8, is set_picard_control's below)
                self.backend.set_kappa_tables(self.kappa_tables, self.picard if self.capacity_form == "lagged" else 1)
            if self.rhoc_tables:
                self.backend.set_rhoc_tables(self.rhoc_tables)
                if self.capacity_form == "enthalpy":    # (lagged is every context's default: no extra call)
                    self.backend.set_capacity_form("enthalpy")
                    self.backend.set_picard_control(self.picard_tol or 0.0, self.picard_relax, self.picard)
                else:
                    self.backend.set_picard(self.picard)
            self.backend.set_state(u)
            self.backend.assemble(self.dt, self.assembly_mode)
        else:
            self.backend.assemble(self.dt, self.assembly_mode)
            self.backend.set_state(u)
        self.setup_seconds = time.perf_counter() - t0
        self.iters = []

    def set_materials(self, tag_to_k, tag_to_rho_cv, assemble=True):
        """(Re)load the coefficient tables; with ``assemble`` re-value M, A (kappa sweeps reuse
        the mesh, the pattern and the Dirichlet set)."""
        tags = sorted(tag_to_k)
        self._rho_c = {int(t): float(tag_to_rho_cv[t]) for t in tags}      # the constants of the monitors' energy
        self.backend.set_materials(np.array(tags, dtype=np.int32),
                                   np.array([tag_to_k[t] for t in tags], dtype=np.float64),
                                   np.array([tag_to_rho_cv[t] for t in tags], dtype=np.float64))
        if assemble:
            self.backend.assemble(self.dt, self.assembly_mode)

    def picard_change(self):
        """max |u^{n+1,p} - u^{n+1,p-1}| of the last step's last Picard sweep (with tables only)."""
        return self.backend.picard_change()

    def picard_history(self):
        """{"sweeps", "change"}: per step since the problem was made, the sweeps used and the last max |x_k - e_{k-1}| (enthalpy
        form only)."""
        if self.capacity_form != "enthalpy":
            raise ValueError('picard_history: needs capacity_form="enthalpy"')
        sweeps, change = self.backend.picard_history()
        return {"sweeps": sweeps, "change": change}

    def stored_heat(self, T_ref=None):
        """{cell tag: the heat stored in the tag's cells above ``T_ref`` in J}: 2 pi sum_e vol_e (H_tag(Tw_e(u)) - H_tag(T_ref)),
        scaled as the monitors' ``energy`` is (hf_stored_heat).  ``T_ref`` None: the scalar u0 of the problem.
        With any tables or none, under both capacity forms."""
        T_ref = self._heat_T_ref(T_ref)
        rec = self.backend.stored_heat(T_ref)
        return {int(t): 2.0 * np.pi * float(rec[int(t)]) for t in sorted(self._rho_c)}

    def _heat_T_ref(self, T_ref):
        if T_ref is None:
            T_ref = self.monitor_T_ref
        if T_ref is None:
            raise ValueError("stored_heat: T_ref is needed (the problem's u0 is not a scalar)")
        return float(T_ref)

    def clear_picard_history(self):
        self.backend.clear_picard_history()

    def clear_heat_history(self):
        self.backend.clear_heat_records()

    def record_heat(self, on=True, T_ref=None):
        """Keep one stored-heat record per step of :meth:`step` / :meth:`run` from now on (hf_set_heat_records)."""
        self.backend.set_heat_records(bool(on), self._heat_T_ref(T_ref) if on else 0.0)

    def heat_history(self, first=0, count=None):
        """{cell tag: array}: the stored heat (J, as :meth:`stored_heat`) after every recorded step (:meth:`record_heat`)."""
        rec = self.backend.get_heat(first, count)
        return {int(t): 2.0 * np.pi * rec[:, int(t)] for t in sorted(self._rho_c)}

    def close(self):
        if self._own_backend:
            self.backend.close()

    # -- boundary values -------------------------------------------------------------------
    def bc_values(self, t, only=None):
        """g_B(t).  ``only`` = BCs to refresh (the reference refreshes all once at t=0 and then
        only the heated line, run_with_diamond.py:458-459, 472)."""
        for bc in (self.bcs if only is None else only):
            bc.update(t)
        if getattr(self, "_plan", None) is None or len(self._plan) != len(self.bcs):
            self._plan = gather_plan(len(self.bcs), self._owner, self._pos)
        return gather_bc_values(self.bcs, self._owner, self._pos, self._plan)

    # -- stepping --------------------------------------------------------------------------
    def set_state(self, u):
        u = np.full(self.n, float(u)) if np.isscalar(u) else u
        self.backend.set_state(u)

    def state(self):
        return self.backend.get_state()

    # -- region monitors -------------------------------------------------------------------
    def _combine_monitors(self, records):
        if not self.monitors:
            raise ValueError("monitors: the problem has no monitors (HeatProblem(..., monitors=))")
        return combine_monitors(records, self.monitors, self.coords, rho_c=self._rho_c, T_ref=self.monitor_T_ref,
                                tabled=self.rhoc_tables)

    def monitors_now(self):
        """{region: {field: value}} of the current state (heatflow_amd.monitors for the fields); nothing is recorded."""
        if not self.monitors:
            raise ValueError("monitors: the problem has no monitors (HeatProblem(..., monitors=))")
        return self._combine_monitors(self.backend.monitor_now())

    def monitor_history(self, first=0, count=None):
        """{region: {field: array}}: one value per recorded step (every step of step / run / run_tangent since the problem was
        made or :meth:`clear_monitor_history` was called), from record ``first`` on."""
        if not self.monitors:
            raise ValueError("monitors: the problem has no monitors (HeatProblem(..., monitors=))")
        return self._combine_monitors(self.backend.get_monitors(first, count))

    def clear_monitor_history(self):
        if self.monitors:
            self.backend.clear_monitor_records()

    def source_vector(self):
        """F1 of the source: the load at unit amplitude (n values; 2 pi sum(F1) = the power in W per unit amplitude)."""
        return self.backend.get_source()

    def source_derivative(self, which):
        """dF1/dfwhm (``which`` = "fwhm") or dF1/ddepth ("depth") of the source (n values); makes the source
        differentiable if it is not yet."""
        if not self.source:
            raise ValueError("source_derivative: the problem has no source (HeatProblem(..., source=))")
        if which not in ("fwhm", "depth"):
            raise ValueError(f"source_derivative: 'fwhm' or 'depth' expected, got {which!r}")
        if not self._source_diff:
            self.backend.source_derivatives(True)
            self._source_diff = True
        return self.backend.get_source_derivative(which)

    def _source_amplitudes(self, source_amplitude, times):
        """The amplitudes of the steps that end at ``times``: a callable p(t), or one value per step."""
        if not self.source:
            raise ValueError("source_amplitude: the problem has no source (HeatProblem(..., source=))")
        if callable(source_amplitude):
            p = np.array([float(source_amplitude(float(t))) for t in times], dtype=np.float64)
        else:
            p = np.asarray(source_amplitude, dtype=np.float64).ravel()
        if p.shape != (len(times),):
            raise ValueError(f"source_amplitude: {len(times)} values expected, got {p.shape[0]}")
        if not np.all(np.isfinite(p)):
            raise ValueError("source_amplitude: every amplitude must be finite")
        return p

    def step(self, t, only=None, source_amplitude=None):
        """One step to time ``t``.  With a source, ``source_amplitude`` = p(t) or the value itself (None: 0)."""
        if self.source:
            self.backend.set_source_amplitudes([] if source_amplitude is None else self._source_amplitudes(source_amplitude, [t]))
        elif source_amplitude is not None:
            self._source_amplitudes(source_amplitude, [t])
        g = self.bc_values(t, only)
        it, res = self.backend.step(g, self.rtol, self.atol, self.max_it)
        self.iters.append(it)
        return it, res

    def run(self, num_steps, watcher_nodes=None, time_varying=None, first_step=0, source_amplitude=None):
        """``num_steps`` steps t_k = (k+1) dt in one backend call (hf_run): the boundary values
        of all steps are tabulated on the host first.  Returns (times, samples, iters).  With a source,
        ``source_amplitude`` = a callable p(t) evaluated at (k+1) dt or one value per step, in W/m^3 (None: amplitude 0)."""
        for bc in self.bcs:
            bc.update(0.0)
        times = (np.arange(first_step, first_step + num_steps) + 1) * self.dt
        if self.source:
            self.backend.set_source_amplitudes([] if source_amplitude is None else self._source_amplitudes(source_amplitude, times))
        elif source_amplitude is not None:
            self._source_amplitudes(source_amplitude, times)
        g_all = np.empty((num_steps, len(self.bc_dofs)), dtype=np.float64)
        for k, t in enumerate(times):
            g_all[k] = self.bc_values(t, time_varying)
        samples, iters = self.backend.run(g_all, self.rtol, self.atol, self.max_it, watcher_nodes)
        self.iters.extend(int(i) for i in iters)
        return times, samples, iters

    # -- variable time steps ------------------------------------------------------
    def _varstep_refusals(self, what):
        if self.capacity_form == "enthalpy":
            raise ValueError(f'{what}: capacity_form="enthalpy" is not supported (its sweeps take the assembled step)')
        if self.assembly_mode != ASM_ROW_GATHER:
            raise ValueError(f"{what}: needs assembly_mode=ASM_ROW_GATHER (the operator is re-valued by the row-gather kernel)")

    def _consistent_start(self, t, time_varying):
        """The state's Dirichlet entries take the boundary values of the time ``t``.  Every step overwrites those entries; what
        this changes is the first right-hand side M u^n, where the consistent mass matrix couples them to the neighbouring rows:
        a drive that is not exactly zero at the start would otherwise enter as a jump of the boundary, to which those rows respond
        by a fixed fraction of the jump at any step size - an error no step size resolves."""
        if float(self.backend.step_info()["t"]) != 0.0:
            raise ValueError("consistent start: the run is already under way (the state would be set again, which puts the "
                             "backend's time record and BDF2's history back to rest); start from set_state or solve_steady")
        g = self.bc_values(t, time_varying)
        if len(self.bc_dofs):
            u = self.backend.get_state()
            u[self.bc_dofs] = g
            self.backend.set_state(u)

    def _restore_step(self):
        """The following steps have the assembled size ``dt`` again (hf_set_step is sticky: without this a later :meth:`run` or
        :meth:`step`, which tabulate their boundary values at multiples of ``dt``, would step with the last variable size).  Under
        BDF2 the library refuses a step more than 1 + sqrt 2 times the one before it; where ``dt`` is that much larger than the
        last step taken (a run that ended on a short step, or left through NotConverged) the state is set again, so that the
        next step starts from rest - first order for one step, instead of an unstable ratio."""
        try:
            self.backend.set_step(self.dt)
        except ValueError:
            self.backend.set_state(self.backend.get_state())
            self.backend.set_step(self.dt)

    def run_steps(self, dts, watcher_nodes=None, time_varying=None, source_amplitude=None, t_start=None, consistent_start=False):
        """One step per entry of ``dts`` (s) in one backend call (hf_set_step_list + hf_run): the operator is re-valued on the GPU
        whenever the effective step changes.  Boundary values and source amplitudes are tabulated at the step ends
        ``t_start + cumsum(dts)`` (``t_start`` None: the backend's time record, 0 after the set-up, set_state or solve_steady).
        BDF2 refuses a step more than 1 + sqrt 2 times the one before.  Afterwards the list is cleared and later steps have the
        assembled size ``dt`` again (see _restore_step).  ``consistent_start``: the state's Dirichlet entries first take the boundary values of the start time
        (as :meth:`run_adaptive` does; the state is set again, so the run starts at rest).  Returns (times, samples, iters)."""
        self._varstep_refusals("run_steps")
        dts = np.asarray(dts, dtype=np.float64).ravel()
        if dts.size == 0 or not (np.all(np.isfinite(dts)) and np.all(dts > 0.0)):
            raise ValueError("run_steps: dts must be a non-empty list of positive, finite step sizes")
        t0 = float(self.backend.step_info()["t"]) if t_start is None else float(t_start)
        times = np.cumsum(np.concatenate([[t0], dts]))[1:]
        for bc in self.bcs:
            bc.update(0.0)
        if consistent_start:
            self._consistent_start(t0, time_varying)
        if self.source:
            self.backend.set_source_amplitudes([] if source_amplitude is None else self._source_amplitudes(source_amplitude, times))
        elif source_amplitude is not None:
            self._source_amplitudes(source_amplitude, times)
        g_all = np.empty((len(dts), len(self.bc_dofs)), dtype=np.float64)
        for k, t in enumerate(times):
            g_all[k] = self.bc_values(t, time_varying)
        self.backend.set_step_list(dts)
        try:
            samples, iters = self.backend.run(g_all, self.rtol, self.atol, self.max_it, watcher_nodes)
        finally:
            self.backend.set_step_list([])
            self._restore_step()
        self.iters.extend(int(i) for i in iters)
        return times, samples, iters

    def run_adaptive(self, t_final, tol, watcher_nodes=None, time_varying=None, dt_init=None, dt_min=None, dt_max=None, atol=None,
                     rtol=0.0, source_amplitude=None, safety=0.9, shrink=0.25, grow=2.0, keep=(1.0, 1.2), on_accept=None):
        """Steps of controlled size from the backend's current time (0 after the set-up, set_state or solve_steady; the run starts
        at rest) to ``t_final``: hf_step, then the local-error indicator of the step (hf_get_step_error: max over the free rows of
        |estimate| / (atol + rtol |u|), ``atol`` None = ``tol``), then the controller of :mod:`heatflow_amd.stepping` accepts the
        step or undoes it (hf_step_reject) and proposes the next size.  The last step lands on ``t_final``.  ``dt_init`` None:
        (t_final - t) / 400.  The state's Dirichlet entries first take the boundary values of the start time (a drive that is not
        exactly zero there must not enter as a jump: see _consistent_start).  ``source_amplitude``: a callable p(t).  The indicator is conservative (it overstates the true local
        error 1.3 x to 2 x on the stock small mesh), not a bound, and it reads every kink of a data-driven boundary curve as error:
        adaptive steps pay off under smooth drives only.  Raises NotConverged when a step of ``dt_min`` is still
        rejected.  Returns (times, samples, iters, info), info = {"accepted", "rejected", "revaluations", "dt", "err"} with the
        accepted sizes and their estimates (in units of ``tol``'s, i.e. K with the default atol).  ``on_accept(t)`` is called after
        every accepted step, with the state in place (the drivers' field sink)."""
        from .hip_backend import HF_ERR_NOCONV, NotConverged
        from .stepping import StepController, scheme_order

        self._varstep_refusals("run_adaptive")
        if source_amplitude is not None and not callable(source_amplitude):
            raise ValueError("run_adaptive: source_amplitude must be a callable p(t) (the step ends are not known beforehand)")
        be = self.backend
        t = float(be.step_info()["t"])
        t_final = float(t_final)
        if not t_final > t:
            raise ValueError(f"run_adaptive: t_final {t_final!r} is not ahead of the current time {t!r}")
        ctrl = StepController(float(tol), scheme_order(self.scheme), safety=safety, shrink=shrink, grow=grow, keep=keep,
                              dt_min=dt_min, dt_max=dt_max)
        atol = float(tol) if atol is None else float(atol)
        dt = ctrl.limit((t_final - t) / 400.0 if dt_init is None else float(dt_init))
        nodes = None if watcher_nodes is None or len(watcher_nodes) == 0 else np.asarray(watcher_nodes, dtype=np.int32)
        for bc in self.bcs:
            bc.update(0.0)
        self._consistent_start(t, time_varying)
        reval0 = be.step_info()["revaluations"]
        times, samples, iters, dts, errs = [], [], [], [], []
        rejected = 0
        be.set_step_control(True)
        try:
            while True:
                h, lands = ctrl.toward(t, dt, t_final)
                t_new = t_final if lands else t + h
                be.set_step(h)
                if self.source:
                    be.set_source_amplitudes([] if source_amplitude is None else self._source_amplitudes(source_amplitude, [t_new]))
                it, _ = be.step(self.bc_values(t_new, time_varying), self.rtol, self.atol, self.max_it)
                self.iters.append(int(it))
                err = be.step_error(atol, float(rtol)) * ctrl.tol
                ok, dt_next = ctrl.decide(err, h)
                if not ok:
                    be.step_reject()
                    rejected += 1
                    if ctrl.at_floor(h):
                        raise NotConverged(HF_ERR_NOCONV, f"run_adaptive: a step of dt_min = {ctrl.dt_min:.3e} s at t = {t:.6e} s "
                                                          f"is still rejected (estimate {err:.3e} against tol {ctrl.tol:.3e})")
                    dt = dt_next
                    continue
                t = t_new
                times.append(t)
                iters.append(int(it))
                dts.append(h)
                errs.append(err)
                if nodes is not None:
                    samples.append(be.sample(nodes))
                if on_accept is not None:
                    on_accept(t)
                if lands:
                    break
                dt = dt_next if h == dt else max(dt_next, min(dt, ctrl.grow * h))   # (a step shortened to split the rest does not hold the size back)
        finally:
            be.set_step_control(False)
            self._restore_step()
        info = {"accepted": len(dts), "rejected": rejected, "revaluations": be.step_info()["revaluations"] - reval0,
                "dt": np.array(dts), "err": np.array(errs)}
        samp = np.array(samples) if nodes is not None else np.empty((len(dts), 0))
        return np.array(times), samp, np.array(iters, dtype=np.int32), info

    def run_tangent(self, num_steps, watcher_nodes, conductivity=(), boundary=None, time_varying=None, first_step=0, shape=None,
                    capacity=(), monitor_tangents=False, source_amplitude=None, source=None, tables=None):
        """:meth:`run` plus the derivatives of the watcher curves with respect to parameters theta_j (hf_run_tangent,
        DESIGN.md 3.7).  Column j of ``conductivity`` = the cell tags whose conductivity theta_j is (they move together).  An
        entry may also be a pair ``(tag, "k" | "r" | "z")``: the tag's kappa (both directions of an anisotropic
        tag, their ratio kept), its k_r or its k_z in W/m/K; one tag may give its k_r to one column and its k_z to another.  Plain
        tags only make the set-up of before (hf_tangent_setup, which refuses anisotropic tags), any pair hf_tangent_setup_dir;
        ``boundary`` = {column: {bc index: dg/dtheta_j callable (x, y, t)}} for parameters that enter the Dirichlet values
        (e.g. ``HeatingCurve.gaussian_dfwhm`` on the heated line).  A column may be both.  The derivatives are tabulated
        exactly as :meth:`run` tabulates g.  The first call after a set-up starts every tangent at zero, later calls
        continue them (as the state continues).  The tangents start at zero, i.e. the initial state is taken as independent
        of the parameters: after :meth:`solve_steady` (whose answer depends on the conductivities) the backend refuses a
        tangent run until :meth:`set_state`.  ``shape`` = {column: vz} makes a column (also) a shape column:
        the nodes move along z with the nodal velocity vz = dz / dtheta_j (n values, e.g. geometry.thickness_velocity at the
        nodes' z), the triangles stay, and the column's tangent is the derivative at the moving nodes (hf_tangent_set_shape, at
        most 4 columns).  Without ``shape`` the backend sees the calls of before.  Column j of ``capacity`` (positional like
        ``conductivity``; an empty list = none) = the cell tags whose rho_c = rho * cv in J/m^3/K theta_j is (DESIGN.md 3.16,
        hf_tangent_set_capacity); a column may carry conductivities, a velocity and a capacity at once, a tag may be in one
        capacity column only, and without ``capacity`` the backend sees the calls of before.  ``monitor_tangents`` (DESIGN.md
        3.18; needs ``monitors=``) switches the derivative records of the region monitors on for this run:
        :meth:`monitor_tangent_history` then gives the derivative of every monitor field along every column, per step; the
        default makes no new backend call.  ``source`` (needs ``source=`` on the problem) makes the problem's
        source differentiable, after which the backend accepts a tangent run under it (``{}`` is enough; without the keyword a
        problem with a source is refused as before), and gives the source columns: {column: {"amplitude": c0, "fwhm": c1, "depth":
        c2}}, each one value per step or a callable of time (missing: 0), adds c0 F1 + c1 G_f + c2 G_d = d(p_k F1)/dtheta_j to the
        column's load at step k (heatflow_amd.source.tangent_coefficients gives them for the source's own parameters).
        ``source_amplitude`` has the meaning it has in :meth:`run`.  Shape columns under a source are refused.  ``tables``
        (needs ``kappa_tables=`` or ``rhoc_tables=`` on the problem, one Picard sweep) allows the tangent run under
        the tables (``{}`` is enough; without the keyword a problem with tables is refused as before) and gives the columns their
        derivative tables: {column: {"kappa": {cell tag: values}, "rhoc": {cell tag: values}}}, values = d(knot value)/dtheta_j at
        the knots of the tag's table (heatflow_amd.kappa_t.table_derivative gives them for the parameters of a material).  Every
        column, with or without such a table, feels the tables through the coupling term kappa'(T) s.  Conductivity columns on
        tags with a conductivity table, capacity columns on tags with a capacity table, shape columns, a source and
        ``monitor_tangents`` are refused under ``tables``.  Returns (times, samples, tangent samples (n_steps, n_par, n_s), iters, tangent iters
        (n_steps, n_par))."""
        if monitor_tangents and not self.monitors:
            raise ValueError("run_tangent: monitor_tangents needs monitors (HeatProblem(..., monitors=))")
        conductivity = [list(c) for c in conductivity]
        boundary = {int(j): dict(m) for j, m in (boundary or {}).items()}
        shape = {int(j): np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for j, v in (shape or {}).items()}
        for j, v in shape.items():
            if j < 0 or v.shape != (self.n,):
                raise ValueError(f"run_tangent: shape column {j}: {self.n} velocities expected (got {v.size})")
        cap_col = {}
        for j, tags in enumerate(capacity or ()):
            for t in tags:
                if int(t) in cap_col:
                    raise ValueError(f"run_tangent: cell tag {t} is listed in two capacity columns")
                cap_col[int(t)] = j
        if source is None and source_amplitude is not None:
            raise ValueError("run_tangent: source_amplitude needs source= (tangents under a source are switched on by it)")
        if source is not None and not self.source:
            raise ValueError("run_tangent: source= needs a source (HeatProblem(..., source=))")
        if source is not None and shape:
            raise ValueError("run_tangent: shape columns under a source are not supported (the source's load depends on the "
                             "node positions)")
        if tables is not None and not (self.kappa_tables or self.rhoc_tables):
            raise ValueError("run_tangent: tables= needs tables (HeatProblem(..., kappa_tables= / rhoc_tables=))")
        if tables is not None and self.picard > 1:
            raise ValueError(f"run_tangent: tables= covers the lagged scheme only (picard = 1, not {self.picard})")
        if tables is not None and (shape or source is not None or monitor_tangents):
            raise ValueError("run_tangent: tables= together with " + ("shape" if shape else "source" if source is not None
                                                                      else "monitor_tangents") + " is not supported")
        tab_cols = {0: {}, 1: {}}
        for j, kinds in (tables or {}).items():
            unknown = sorted(set(kinds) - {"kappa", "rhoc"})
            if int(j) < 0 or unknown:
                raise ValueError(f"run_tangent: tables column {j}: " + (f"unknown key {unknown[0]!r} (kappa, rhoc)"
                                                                        if unknown else "a negative column"))
            for q, key in enumerate(("kappa", "rhoc")):
                own = {int(t): v for t, v in (self.kappa_tables if q == 0 else self.rhoc_tables).items()}
                for t, v in (kinds.get(key) or {}).items():
                    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
                    if int(t) not in own or v.shape != np.shape(own[int(t)][2]):
                        raise ValueError(f"run_tangent: tables column {j}: cell tag {t} has no {key} table of {v.size} knots")
                    tab_cols[q][(int(j), int(t))] = v
        src_cols = {}
        for j, parts in (source or {}).items():
            unknown = sorted(set(parts) - set(SOURCE_COLUMN_KEYS))
            if int(j) < 0 or unknown:
                raise ValueError(f"run_tangent: source column {j}: " + (f"unknown key {unknown[0]!r} (amplitude, fwhm, depth)"
                                                                        if unknown else "a negative column"))
            src_cols[int(j)] = dict(parts)
        n_par = max([len(conductivity), len(capacity or ())] + [j + 1 for j in boundary] + [j + 1 for j in shape]
                    + [j + 1 for j in src_cols] + [j + 1 for q in tab_cols for j, _ in tab_cols[q]])
        if n_par == 0:
            raise ValueError("run_tangent: no parameter (conductivity, boundary, shape, source or tables) given")
        directional = any(isinstance(t, (tuple, list)) for tags in conductivity for t in tags)
        if not directional:
            tag_col = {}
            for j, tags in enumerate(conductivity):
                for t in tags:
                    if int(t) in tag_col:
                        raise ValueError(f"run_tangent: cell tag {t} is listed in two conductivity columns")
                    tag_col[int(t)] = j
            spec = (n_par, tuple(sorted(tag_col.items())))
        else:
            cols = {"k": {}, "r": {}, "z": {}}
            for j, tags in enumerate(conductivity):
                for t in tags:
                    t, kind = (t[0], str(t[1])) if isinstance(t, (tuple, list)) else (t, "k")
                    if kind not in cols:
                        raise ValueError(f"run_tangent: cell tag {t}: unknown kind {kind!r} ('k', 'r' or 'z')")
                    t = int(t)
                    if t in cols[kind]:
                        raise ValueError(f"run_tangent: cell tag {t} is listed in two conductivity columns ({kind})")
                    if (t in cols["k"]) if kind != "k" else (t in cols["r"] or t in cols["z"]):
                        raise ValueError(f"run_tangent: cell tag {t} has a kappa column and a directional one")
                    cols[kind][t] = j
            spec = (n_par, "dir") + tuple(tuple(sorted(cols[q].items())) for q in ("k", "r", "z"))
        if shape:
            spec += ("shape",) + tuple((j, hashlib.sha1(shape[j].tobytes()).hexdigest()) for j in sorted(shape))
        if cap_col:
            spec += ("capacity",) + tuple(sorted(cap_col.items()))
        if src_cols:
            spec += ("source",) + tuple(sorted(src_cols))
        if tables is not None:
            spec += ("tables",) + tuple((q, key, hashlib.sha1(tab_cols[q][key].tobytes()).hexdigest())
                                        for q in tab_cols for key in sorted(tab_cols[q]))
            if not getattr(self, "_table_deriv", False):
                self.backend.table_derivatives(True)             # (before the set-up, which refuses tables without it)
                self._table_deriv = True
                self._tangent_spec = None                        # (the call dropped the set-up)
        if source is not None and not self._source_diff:
            self.backend.source_derivatives(True)            # (before the set-up, which refuses a source that is not differentiable)
            self._source_diff = True
        if getattr(self, "_tangent_spec", None) != spec:     # a new set of parameters: the tangents start from zero
            if directional:
                self.backend.tangent_setup_dir(n_par, cols["k"], cols["r"], cols["z"])
            else:
                self.backend.tangent_setup(n_par, tag_col)
            if cap_col:                                      # (the set-up removed whatever capacity columns were there)
                self.backend.tangent_set_capacity(cap_col)
            for j in sorted(shape):                          # (the set-up removed whatever velocities were there)
                self.backend.tangent_set_shape(j, shape[j])
            for q in (0, 1):                                 # (and whatever derivative tables)
                if tab_cols[q]:
                    self.backend.tangent_set_tables(q, tab_cols[q])
            self._tangent_spec = spec
        nv = self.backend.tangent_nv
        for bc in self.bcs:
            bc.update(0.0)
        times = (np.arange(first_step, first_step + num_steps) + 1) * self.dt
        if source is not None:
            self.backend.set_source_amplitudes([] if source_amplitude is None else self._source_amplitudes(source_amplitude, times))
            if src_cols:
                coef = np.zeros((num_steps, nv, 3), dtype=np.float64)
                for j, parts in src_cols.items():
                    for q, key in enumerate(SOURCE_COLUMN_KEYS):
                        if parts.get(key) is not None:
                            coef[:, j, q] = self._source_amplitudes(parts[key], times)
                self.backend.tangent_set_source(coef)
        g_all = np.empty((num_steps, len(self.bc_dofs)), dtype=np.float64)
        h_all = np.zeros((num_steps, len(self.bc_dofs), nv), dtype=np.float64) if boundary else None
        for k, t in enumerate(times):
            g_all[k] = self.bc_values(t, time_varying)
            for j, per_bc in boundary.items():
                for q, deriv in per_bc.items():
                    bc = self.bcs[q]
                    sel, src = self._plan[q]
                    if sel.size == 0:
                        continue
                    te = t if (time_varying is None or any(bc is b for b in time_varying)) else 0.0
                    h_all[k, sel, j] = _eval_on_dofs(deriv, bc.dof_coords, te)[src]
        if monitor_tangents:
            first = self.backend.monitor_tangent_count()[0]      # (a set-up with another nv has dropped the records of before)
            self.backend.set_monitor_tangents(True)
        try:
            samples, iters, tsamples, titers = self.backend.run_tangent(g_all, h_all, self.rtol, self.atol, self.max_it,
                                                                        watcher_nodes)
        finally:
            if monitor_tangents:
                self.backend.set_monitor_tangents(False)
        if monitor_tangents:     # this run's derivative records, its columns and the tags whose rho_c they carry (energy's explicit term)
            self._mt_run = (first, num_steps, n_par, dict(cap_col))
        self.iters.extend(int(i) for i in iters)
        return times, samples, tsamples[:, :n_par], iters, titers[:, :n_par]

    def monitor_tangent_history(self, scale=None):
        """{region: {field: array (n_steps, n_par)}}: the derivatives of the monitor fields T_max, T_min, volume, T_mean,
        hot_volume, hot_fraction and energy along the columns of the last :meth:`run_tangent` with ``monitor_tangents=True``, one
        row per step (heatflow_amd.monitors.combine_tangents; ``scale`` multiplies whole columns)."""
        if not self.monitors:
            raise ValueError("monitors: the problem has no monitors (HeatProblem(..., monitors=))")
        if getattr(self, "_mt_run", None) is None:
            raise ValueError("monitor_tangents: no tangent run with monitor_tangents=True yet")
        first, count, n_par, cap_col = self._mt_run
        drec, index = self.backend.get_monitor_tangents(first, count)
        rec = self.backend.get_monitors()[np.asarray(index, dtype=np.int64)]
        return combine_tangents(rec, drec[:, :, :n_par], self.monitors, rho_c=self._rho_c, T_ref=self.monitor_T_ref,
                                tabled=self.rhoc_tables, capacity_columns=cap_col, scale=scale)

    def tangent(self, j):
        """The current tangent field of column j (n values)."""
        return self.backend.get_tangent(j)

    def tangent_load(self, j):
        """The load F_j = -K_j u of column j at the current state, by the tangent set-up in force (tests and diagnostics); under
        ``tables=`` the tables' term is included, formed from the columns as they stand."""
        return self.backend.tangent_load(j)


    # -- steady state and pre-heated transients (with_ir_steady.ipynb cells 17-23) -------------
    def solve_steady(self, bcs=None, t=0.0, use_load=False, picard_tol=1e-6, max_sweeps=50):
        """Steady state K u = F with its own Dirichlet list ``bcs`` (default: the problem's), merged last-wins and
        evaluated at ``t``; K is the r-weighted stiffness of the transient operator (steady state), F the
        load when ``use_load`` and one is set, else 0.  The answer becomes the state.  Returns (u, iters, resid).
        :meth:`run_tangent` refuses the steady state (HF_ERR_STATE) until :meth:`set_state`: it depends on the
        conductivities, and the tangents of a run start at zero.
        With ``kappa_tables`` or ``rhoc_tables`` the steady state is nonlinear: a Picard iteration from the current state
         until max |x_k - x_{k-1}| <= ``picard_tol``, at most ``max_sweeps`` sweeps (NotConverged beyond).  Then
        ``iters`` is the sum over the sweeps, ``resid`` the relative residual of the nonlinear problem at the answer, and
        ``steady_info`` holds {"sweeps", "iters" per sweep, "change", "nl_resid"}."""
        bcs = self.bcs if bcs is None else list(bcs)
        if not bcs:
            raise ValueError("solve_steady: no Dirichlet condition (the stiffness alone is singular)")
        dofs, owner, pos = merge_bcs(bcs)
        for bc in bcs:
            bc.update(t)
        g = gather_bc_values(bcs, owner, pos)
        if self.kappa_tables or self.rhoc_tables:
            self.backend.steady_picard_setup(dofs, self.precond)
            info = self.backend.steady_picard_solve(g, use_load, self.rtol, self.atol, self.max_it, picard_tol, max_sweeps)
            self.steady_info = info
            return self.backend.get_state(), sum(info["iters"]), info["nl_resid"]
        self.backend.steady_setup(dofs, self.precond)
        it, res = self.backend.steady_solve(g, use_load, self.rtol, self.atol, self.max_it)
        return self.backend.get_state(), it, res

    def set_load(self, F):
        """Load term of every following step, b = M u^n + dt F (BDF2: M (4/3 u^n - 1/3 u^{n-1}) + 2/3 dt F; n values); None
        removes it."""
        self.backend.set_load(None if F is None else np.asarray(F, dtype=np.float64))

    def hold_load(self):
        """The load that holds the current state (the notebook's b_equiv = A_free u_ss): (K u)_i off the problem's merged
        Dirichlet rows, 0 on them; it becomes the load and is returned.  Needs a solve_steady before (for K)."""
        self.backend.hold_load()
        return self.backend.get_load()


SOURCE_COLUMN_KEYS = ("amplitude", "fwhm", "depth")     # c0, c1, c2 of a source column (run_tangent's source=)


def check_source(source):
    """dict(tags, fwhm, z0, depth) of a volumetric source with int tags and float numbers (depth absent or None: inf), or None;
    ValueError for an unknown key, no tag, a tag listed twice, or a number hf_set_source would refuse (before any backend
    call)."""
    if source is None:
        return None
    src = dict(source)
    unknown = sorted(set(src) - {"tags", "fwhm", "z0", "depth"})
    if unknown:
        raise ValueError(f"source: unknown key {unknown[0]!r} (tags, fwhm, z0, depth)")
    for key in ("tags", "fwhm", "z0"):
        if key not in src:
            raise ValueError(f"source: {key} is missing")
    tags = [int(t) for t in np.atleast_1d(src["tags"])]
    if not tags or len(set(tags)) != len(tags):
        raise ValueError(f"source: tags must name at least one cell tag, each once (got {tags!r})")
    fwhm, z0 = float(src["fwhm"]), float(src["z0"])
    depth = float("inf") if src.get("depth") is None else float(src["depth"])
    if not (np.isfinite(fwhm) and fwhm > 0.0):
        raise ValueError(f"source: fwhm must be positive and finite, got {fwhm!r}")
    if not np.isfinite(z0):
        raise ValueError(f"source: z0 must be finite, got {z0!r}")
    if not depth > 0.0:
        raise ValueError(f"source: depth must be positive (or inf for a uniform layer), got {depth!r}")
    return {"tags": tags, "fwhm": fwhm, "z0": z0, "depth": depth}


def check_capacity_form(form, picard, picard_tol, picard_relax, *, scheme="backward_euler", rhoc_tables=None, k_aniso=None):
    """(form, tol or None, relax) of HeatProblem's capacity_form / picard_tol / picard_relax; ValueError (naming the argument)
    for an unknown form, the combinations the enthalpy form does not cover, a cap outside 1..64, a negative tolerance, a
    relaxation outside (0, 1], and for a tolerance or relaxation under the lagged form - before any backend call."""
    if form not in ("lagged", "enthalpy"):
        raise ValueError(f"capacity_form: 'lagged' or 'enthalpy' expected, got {form!r}")
    tol = None if picard_tol is None else float(picard_tol)
    relax = float(picard_relax)
    if form == "lagged":
        if tol is not None or relax != 1.0:
            raise ValueError('picard_tol / picard_relax need capacity_form="enthalpy" (the lagged form takes a fixed number of sweeps)')
        return form, None, 1.0
    if not rhoc_tables:
        raise ValueError('capacity_form="enthalpy" needs rhoc_tables (it is the form of the tabled capacity)')
    if scheme != "backward_euler":
        raise ValueError(f'capacity_form="enthalpy" with scheme={scheme!r} is not supported (backward Euler only)')
    if k_aniso:
        raise ValueError('capacity_form="enthalpy" with k_aniso is not supported (the enthalpy kernel is isotropic)')
    if not 1 <= int(picard) <= 64:
        raise ValueError(f'picard: the sweep cap of capacity_form="enthalpy" is 1..64, got {picard!r}')
    if tol is not None and not (tol >= 0.0 and np.isfinite(tol)):
        raise ValueError(f"picard_tol: a tolerance >= 0 in K expected, got {picard_tol!r}")
    if not (0.0 < relax <= 1.0):
        raise ValueError(f"picard_relax: a factor in (0, 1] expected, got {picard_relax!r}")
    return form, tol, relax


def check_k_aniso(k_aniso):
    """{cell tag: (m_r, m_z)} with int tags and float pairs; ValueError for anything that is not a pair of positive finite
    numbers (before any backend call)."""
    out = {}
    for t, v in dict(k_aniso or {}).items():
        try:
            m_r, m_z = (float(x) for x in v)
        except (TypeError, ValueError):
            raise ValueError(f"k_aniso: cell tag {t} needs a pair (m_r, m_z), got {v!r}") from None
        if not (np.isfinite(m_r) and np.isfinite(m_z) and m_r > 0.0 and m_z > 0.0):
            raise ValueError(f"k_aniso: multipliers of cell tag {t} must be positive and finite, got {(m_r, m_z)!r}")
        out[int(t)] = (m_r, m_z)
    return out


def _eval_on_dofs(fn, xy, t):
    """fn(x, y, t) on a BC's DOF coordinates: on whole arrays, else point by point (as RowDirichletBC.update)."""
    x, y = xy[:, 0], xy[:, 1]
    try:
        v = np.asarray(fn(x, y, t), dtype=np.float64)
        if v.shape == ():
            v = np.full(x.shape, float(v))
        if v.shape != x.shape:
            raise ValueError
    except (TypeError, ValueError):
        v = np.array([fn(a, b, t) for a, b in zip(x, y)], dtype=np.float64)
    return v


def nearest_nodes(coords, points):
    """Nearest mesh node of each (z, r) point (run_with_diamond.py:443-449 asks a cKDTree over geometry.x[:, :2] for it).
    A handful of watcher points does not repay a tree over the whole mesh (60 ms to build at 2e5 nodes, plus the import of
    scipy.spatial): one pass of squared distances per point; of equidistant nodes the lowest-numbered one is taken."""
    xy = np.asarray(coords, dtype=np.float64)[:, :2]
    out = np.empty(len(points), dtype=np.int32)
    for q, p in enumerate(points):
        dz, dr = xy[:, 0] - float(p[0]), xy[:, 1] - float(p[1])
        out[q] = int(np.argmin(dz * dz + dr * dr))
    return out
