"""ctypes binding of libheatflow_hip.so (include/heatflow_hip.h).

This is the only device path: there is no CPU fallback.  If the shared library
is missing or no HIP device is present, construction raises ``HipUnavailable``.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HEATFLOW_HIP_LIB") or os.path.join(_HERE, "csrc", "libheatflow_hip.so")  # env: A/B builds

HF_OK, HF_ERR_ARG, HF_ERR_STATE, HF_ERR_HIP, HF_ERR_NOCONV, HF_ERR_ALLOC = 0, -1, -2, -3, -4, -5
ASM_LDS_ATOMIC, ASM_LDS_COLORED, ASM_GLOBAL_ATOMIC, ASM_ROW_GATHER = 0, 1, 2, 3
PC_JACOBI, PC_AMG = 0, 1
K_SPMV, K_PCG_SPMV, K_PCG_UPDATE, K_PCG_DIR, K_ASSEMBLE, K_RHS, K_STREAM_READ = range(7)
BATCH_SHARED, BATCH_PER_COLUMN, BATCH_AFFINE = 0, 1, 2
TIME_BACKWARD_EULER, TIME_BDF2 = 0, 1
TIME_SCHEMES = {"backward_euler": TIME_BACKWARD_EULER, "bdf2": TIME_BDF2}   # config / CLI names


def time_scheme_code(name):
    """The hf_set_time_scheme code of a scheme name ("backward_euler" or "bdf2"); ValueError for anything else."""
    if name not in TIME_SCHEMES:
        raise ValueError(f"unknown time scheme {name!r} (expected one of {sorted(TIME_SCHEMES)})")
    return TIME_SCHEMES[name]

CAPACITY_FORMS = {"lagged": 0, "enthalpy": 1}     # hf_set_capacity_form

EXPORTS = [
    "hf_version", "hf_create", "hf_destroy", "hf_last_error", "hf_set_mesh", "hf_set_mesh_prebuilt", "hf_pattern_export_size",
    "hf_pattern_export", "hf_amg_export_size", "hf_amg_export", "hf_amg_install", "hf_set_materials",
    "hf_update_kappa", "hf_set_dirichlet", "hf_assemble", "hf_set_time_scheme", "hf_set_precond", "hf_set_start_vector", "hf_get_response_solves", "hf_get_amg_info", "hf_get_amg_fallbacks", "hf_set_state", "hf_get_state", "hf_sample", "hf_step", "hf_run",
    "hf_batch_begin", "hf_batch_load_column", "hf_batch_set_affine", "hf_batch_set_state", "hf_batch_get_state", "hf_batch_run", "hf_batch_run_flux", "hf_batch_end",
    "hf_batch_set_source", "hf_batch_get_source", "hf_batch_set_source_amplitudes",
    "hf_batch_set_monitors", "hf_batch_monitor_now", "hf_batch_monitor_count", "hf_batch_get_monitors",
    "hf_set_batch_tables", "hf_batch_set_column_kappa", "hf_batch_revalue", "hf_batch_get_operator",
    "hf_flux_setup", "hf_flux_project", "hf_flux_solve", "hf_flux_sample",
    "hf_steady_setup", "hf_steady_solve", "hf_steady_picard_setup", "hf_steady_picard_solve", "hf_set_load", "hf_get_load", "hf_hold_load",
    "hf_set_source", "hf_get_source", "hf_set_source_amplitudes",
    "hf_source_derivatives", "hf_get_source_derivative", "hf_tangent_set_source",
    "hf_set_monitors", "hf_monitor_now", "hf_monitor_count", "hf_get_monitors", "hf_monitor_clear",
    "hf_set_monitor_tangents", "hf_monitor_tangent_count", "hf_get_monitor_tangents", "hf_monitor_tangent_eval",
    "hf_tangent_setup", "hf_tangent_setup_dir", "hf_tangent_set_shape", "hf_tangent_set_capacity", "hf_table_derivatives", "hf_tangent_set_tables", "hf_tangent_load", "hf_run_tangent", "hf_get_tangent", "hf_set_kappa_tables", "hf_get_picard_change", "hf_set_rhoc_tables", "hf_set_picard",
    "hf_set_capacity_form", "hf_set_picard_control", "hf_get_picard_history", "hf_clear_picard_history", "hf_enthalpy_revalue",
    "hf_stored_heat", "hf_set_heat_records", "hf_heat_count", "hf_get_heat", "hf_clear_heat_records", "hf_set_anisotropy", "hf_set_aniso_tables", "hf_get_sizes", "hf_get_csr", "hf_spmv",
    "hf_set_value_lists", "hf_get_value_lists", "hf_get_projection", "hf_get_flux_system",
    "hf_amg_apply", "hf_batch_apply_precond", "hf_dense_inverse", "hf_time_kernel", "hf_set_profile", "hf_get_profile", "hf_last_gpu_ms",
    "hf_set_step", "hf_set_step_list", "hf_set_step_control", "hf_get_step_error", "hf_step_reject", "hf_get_step_info",
]


class HipUnavailable(RuntimeError):
    """libheatflow_hip.so is not built or no HIP device is usable."""


class HipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"heatflow_hip error {code}: {msg}")
        self.code = code


class NotConverged(HipError):
    pass


def build_library(force=False, verbose=False):
    """Compile csrc/heatflow_hip.hip for gfx950 with hipcc (cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc", "heatflow_hip.hip")
    hdr = os.path.join(_HERE, "..", "include", "heatflow_hip.h")
    if not force and os.path.isfile(LIB_PATH):
        csrc = os.path.join(_HERE, "csrc")
        newest = max([os.path.getmtime(src), os.path.getmtime(hdr)] +
                     [os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc) if f.endswith(".hpp")])
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "libheatflow_hip.so"]
    if force:
        cmd.insert(1, "-B")
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout, res.stderr)
    if res.returncode != 0:
        raise RuntimeError("building libheatflow_hip.so failed:\n" + res.stderr)
    return LIB_PATH


_lib = None


def load_library():
    """dlopen the library and declare the prototypes (no device is touched)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise HipUnavailable(f"{LIB_PATH} not found - run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "or `make -C heatflow_amd/csrc`")
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lib.hf_version.restype = C.c_char_p
    lib.hf_last_error.restype = C.c_char_p
    lib.hf_last_error.argtypes = [vp]
    protos = {
        "hf_create": [C.c_int, C.POINTER(vp)],
        "hf_destroy": [vp],
        "hf_set_mesh": [vp, i32, i32, pd, pi, pi],
        "hf_set_mesh_prebuilt": [vp, i32, i32, pd, pi, pi, vp, i64],
        "hf_pattern_export_size": [vp, C.POINTER(i64)],
        "hf_pattern_export": [vp, vp, i64],
        "hf_amg_export_size": [vp, C.POINTER(i64)],
        "hf_amg_export": [vp, vp, i64],
        "hf_amg_install": [vp, vp, i64],
        "hf_set_materials": [vp, i32, pi, pd, pd],
        "hf_update_kappa": [vp, i32, pi, pd],
        "hf_set_dirichlet": [vp, i32, pi],
        "hf_assemble": [vp, dbl, i32],
        "hf_set_time_scheme": [vp, i32],
        "hf_set_precond": [vp, i32, i32],
        "hf_set_start_vector": [vp, i32],
        "hf_get_response_solves": [vp, C.POINTER(i64)],
        "hf_get_amg_info": [vp, pi, pi, i32, pd, pd],
        "hf_get_amg_fallbacks": [vp, C.POINTER(i64)],
        "hf_set_state": [vp, pd],
        "hf_get_state": [vp, pd],
        "hf_sample": [vp, i32, pi, pd],
        "hf_step": [vp, pd, dbl, dbl, i32, pi, pd],
        "hf_run": [vp, i32, pd, dbl, dbl, i32, i32, pi, pd, pi],
        "hf_set_step": [vp, dbl],
        "hf_set_step_list": [vp, i32, pd],
        "hf_set_step_control": [vp, i32],
        "hf_get_step_error": [vp, dbl, dbl, pd],
        "hf_step_reject": [vp],
        "hf_get_step_info": [vp, pd, pd, pd, C.POINTER(i64)],
        "hf_batch_begin": [vp, i32, i32],
        "hf_batch_load_column": [vp, i32],
        "hf_batch_set_affine": [vp, i32, pi, pd],
        "hf_batch_set_state": [vp, i32, pd],
        "hf_batch_get_state": [vp, i32, pd],
        "hf_batch_run": [vp, i32, pd, dbl, dbl, i32, i32, pi, pd, pi],
        "hf_batch_run_flux": [vp, i32, pd, dbl, dbl, i32, i32, pi, pd, pi, i32, dbl, i32, i32, pi, pd, pi],
        "hf_batch_end": [vp],
        "hf_batch_set_source": [vp, i32, pi, dbl, pd, pd],
        "hf_batch_get_source": [vp, i32, pd],
        "hf_batch_set_source_amplitudes": [vp, i32, pd],
        "hf_batch_set_monitors": [vp, i32],
        "hf_batch_monitor_now": [vp, pd],
        "hf_batch_monitor_count": [vp, pi],
        "hf_batch_get_monitors": [vp, i32, i32, pd],
        "hf_set_batch_tables": [vp, i32],
        "hf_batch_set_column_kappa": [vp, i32, i32, pi, pd],
        "hf_batch_revalue": [vp, i32],
        "hf_batch_get_operator": [vp, i32, pd, pd, pd, pd],
        "hf_flux_setup": [vp],
        "hf_flux_project": [vp, dbl, i32, pd, pd, pi],
        "hf_flux_solve": [vp, i32, dbl, i32, pi],
        "hf_flux_sample": [vp, i32, pi, pd, pd],
        "hf_steady_setup": [vp, i32, pi, i32],
        "hf_steady_solve": [vp, pd, i32, dbl, dbl, i32, pi, pd],
        "hf_steady_picard_setup": [vp, i32, pi, i32],
        "hf_steady_picard_solve": [vp, pd, i32, dbl, dbl, i32, dbl, i32, pi, pi, pd, pd],
        "hf_set_load": [vp, pd],
        "hf_get_load": [vp, pd],
        "hf_hold_load": [vp],
        "hf_set_source": [vp, i32, pi, dbl, dbl, dbl],
        "hf_get_source": [vp, pd],
        "hf_set_source_amplitudes": [vp, i32, pd],
        "hf_source_derivatives": [vp, i32],
        "hf_get_source_derivative": [vp, i32, pd],
        "hf_tangent_set_source": [vp, i32, pd],
        "hf_set_monitors": [vp, i32, pd],
        "hf_monitor_now": [vp, pd],
        "hf_monitor_count": [vp, pi],
        "hf_get_monitors": [vp, i32, i32, pd],
        "hf_monitor_clear": [vp],
        "hf_set_monitor_tangents": [vp, i32],
        "hf_monitor_tangent_count": [vp, pi, pi],
        "hf_get_monitor_tangents": [vp, i32, i32, pd, pi],
        "hf_monitor_tangent_eval": [vp, i32, pd, i32, pi, pd, pd],
        "hf_tangent_setup": [vp, i32, pi],
        "hf_tangent_setup_dir": [vp, i32, pi, pi, pi],
        "hf_tangent_set_shape": [vp, i32, pd],
        "hf_tangent_set_capacity": [vp, i32, pi],
        "hf_table_derivatives": [vp, i32],
        "hf_tangent_set_tables": [vp, i32, i32, pi, pi, pd],
        "hf_tangent_load": [vp, i32, pd],
        "hf_run_tangent": [vp, i32, pd, pd, dbl, dbl, i32, i32, pi, pd, pi, pd, pi],
        "hf_get_tangent": [vp, i32, pd],
        "hf_set_kappa_tables": [vp, i32, pi, pd, pd, pi, pd, i32],
        "hf_get_picard_change": [vp, pd],
        "hf_set_rhoc_tables": [vp, i32, pi, pd, pd, pi, pd],
        "hf_set_picard": [vp, i32],
        "hf_set_capacity_form": [vp, i32],
        "hf_set_picard_control": [vp, dbl, dbl, i32],
        "hf_get_picard_history": [vp, pi, pd, i32, pi],
        "hf_clear_picard_history": [vp],
        "hf_enthalpy_revalue": [vp, pd, pd],
        "hf_stored_heat": [vp, dbl, pd],
        "hf_set_heat_records": [vp, i32, dbl],
        "hf_heat_count": [vp, pi],
        "hf_get_heat": [vp, i32, i32, pd],
        "hf_clear_heat_records": [vp],
        "hf_set_anisotropy": [vp, i32, pi, pd, pd],
        "hf_set_aniso_tables": [vp, i32],
        "hf_get_sizes": [vp, pi, pi, C.POINTER(i64), pi],
        "hf_get_csr": [vp, pi, pi, pd, pd],
        "hf_spmv": [vp, i32, pd, pd],
        "hf_set_value_lists": [vp, i32],
        "hf_get_value_lists": [vp, i32, pi, C.POINTER(i64), pi, pi, pi, pd, C.POINTER(C.c_uint32)],
        "hf_get_projection": [vp, i32, pi, pi, pi, pi, pi, pd, pd, pd, pd],
        "hf_get_flux_system": [vp, i32, pd, pd, pd, pd],
        "hf_amg_apply": [vp, pd, pd, pd],
        "hf_batch_apply_precond": [vp, pd, pd, pd],
        "hf_dense_inverse": [vp, i32, pi, pi, pd, pd, pd, pd, pd],
        "hf_time_kernel": [vp, i32, i32, pd],
        "hf_last_gpu_ms": [vp, pd],
        "hf_set_profile": [vp, i32],
        "hf_get_profile": [vp, pd, C.POINTER(i64)],
    }
    for name, args in protos.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    _lib = lib
    return lib


def projection_sizes():
    """(PROJ_MH, PROJ_MT) of the library: solutions kept in the projection ring of the start vector, slots in all (ring +
    boundary responses).  Needs no device."""
    mh, mt = C.c_int32(), C.c_int32()
    rc = load_library().hf_get_projection(None, -1, C.byref(mh), C.byref(mt), None, None, None, None, None, None, None)
    if rc != HF_OK:
        raise HipError(rc, "hf_get_projection: size query failed")
    return mh.value, mt.value


def blob_address(blob):
    """(address, nbytes) of a blob handed to set_mesh(pattern=) / amg_install: a uint8 numpy array, an ``(address, nbytes)``
    tuple, or any object with ``address`` / ``nbytes`` attributes (a device-resident buffer kept alive by its owner, e.g. the
    tensor a sweep received over RCCL: :class:`heatflow_amd.parameter_sweep.DeviceBlob`)."""
    if isinstance(blob, tuple):
        return int(blob[0]), int(blob[1]), blob
    if hasattr(blob, "address") and hasattr(blob, "nbytes") and not isinstance(blob, np.ndarray):
        return int(blob.address), int(blob.nbytes), blob
    arr = np.ascontiguousarray(blob, dtype=np.uint8)
    return arr.ctypes.data, arr.nbytes, arr


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class HeatflowHIP:
    """One solver context = one HIP device + one stream (not thread-safe)."""

    def __init__(self, device_id=0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        rc = self._lib.hf_create(int(device_id), C.byref(self._ctx))
        if rc != HF_OK:
            msg = self._lib.hf_last_error(self._ctx).decode() if self._ctx else "no usable HIP device"
            if self._ctx:
                self._lib.hf_destroy(self._ctx)
                self._ctx = C.c_void_p()
            raise HipUnavailable(f"hf_create(device {device_id}) failed ({rc}): {msg}")
        self.n = self.n_e = self.n_bc = 0
        self.nnz = 0
        self.batch_nv = 0

    # -- lifetime ------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.hf_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc == HF_OK:
            return
        msg = self._lib.hf_last_error(self._ctx).decode()
        if rc == HF_ERR_NOCONV:
            raise NotConverged(rc, msg)
        if rc == HF_ERR_ARG:
            raise ValueError(f"heatflow_hip: {msg}")
        raise HipError(rc, msg)

    # -- set-up --------------------------------------------------------------------------
    def set_mesh(self, coords, tris, tags, pattern=None):
        """``pattern``: the tables another context exported for the same mesh (:meth:`export_pattern`: a uint8
        array, or ``(address, nbytes)`` of a host or device buffer); they are installed instead of being rebuilt."""
        zr, tri, tag = _f64(coords), _i32(tris), _i32(tags)
        if zr.ndim != 2 or zr.shape[1] != 2 or tri.ndim != 2 or tri.shape[1] != 3 or tag.shape != (tri.shape[0],):
            raise ValueError("set_mesh: coords (n,2), tris (n_e,3), tags (n_e,) expected")
        self.tab_len = int(tag.max()) + 1 if tag.size else 0     # entries of the per-tag tables (hf_tangent_setup)
        self.tangent_nv = 0
        if pattern is None:
            self._check(self._lib.hf_set_mesh(self._ctx, zr.shape[0], tri.shape[0], _pd(zr), _pi(tri), _pi(tag)))
        else:
            addr, nbytes, _keep = blob_address(pattern)
            self._check(self._lib.hf_set_mesh_prebuilt(self._ctx, zr.shape[0], tri.shape[0], _pd(zr), _pi(tri), _pi(tag),
                                                       C.c_void_p(addr), nbytes))
        self._refresh_sizes()

    def pattern_bytes(self):
        nb = C.c_int64()
        self._check(self._lib.hf_pattern_export_size(self._ctx, C.byref(nb)))
        return int(nb.value)

    def export_pattern(self, into=None):
        """The connectivity-derived tables of this context's mesh (CSR pattern, compressed column lists, row-gather
        lists) as one uint8 array, for ``set_mesh(..., pattern=)`` of other contexts.  ``into = (address, nbytes)``
        writes to that host or device buffer instead and returns None."""
        nb = self.pattern_bytes()
        if into is not None:
            if int(into[1]) != nb:
                raise ValueError(f"export_pattern: buffer of {into[1]} bytes, need {nb}")
            self._check(self._lib.hf_pattern_export(self._ctx, C.c_void_p(int(into[0])), nb))
            return None
        blob = np.empty(nb, dtype=np.uint8)
        self._check(self._lib.hf_pattern_export(self._ctx, C.c_void_p(blob.ctypes.data), nb))
        return blob

    def amg_export(self, into=None):
        """The multigrid hierarchy of this context (assembled with PC_AMG) as one uint8 array, for ``amg_install`` of other
        contexts on the same mesh.  ``into = (address, nbytes)`` writes to that host or device buffer and returns None."""
        nb = C.c_int64()
        self._check(self._lib.hf_amg_export_size(self._ctx, C.byref(nb)))
        if into is not None:
            if int(into[1]) != nb.value:
                raise ValueError(f"amg_export: buffer of {into[1]} bytes, need {nb.value}")
            self._check(self._lib.hf_amg_export(self._ctx, C.c_void_p(int(into[0])), nb.value))
            return None
        blob = np.empty(nb.value, dtype=np.uint8)
        self._check(self._lib.hf_amg_export(self._ctx, C.c_void_p(blob.ctypes.data), nb.value))
        return blob

    def amg_install(self, blob):
        """Install a hierarchy another context exported (after set_dirichlet and set_precond(PC_AMG, reuse=True), before
        assemble): nothing is built on the host; assemble() then decides from the blob's fingerprint whether this context's
        operator is the one the hierarchy was built from."""
        addr, nbytes, _keep = blob_address(blob)
        self._check(self._lib.hf_amg_install(self._ctx, C.c_void_p(addr), nbytes))

    def _refresh_sizes(self):
        n, ne, nbc, nnz = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._lib.hf_get_sizes(self._ctx, C.byref(n), C.byref(ne), C.byref(nnz), C.byref(nbc)))
        self.n, self.n_e, self.nnz, self.n_bc = n.value, ne.value, nnz.value, nbc.value

    def set_materials(self, tags, kappa, rho_c):
        t, k, c = _i32(tags), _f64(kappa), _f64(rho_c)
        if not (t.shape == k.shape == c.shape) or t.ndim != 1:
            raise ValueError("set_materials: three 1-D arrays of equal length expected")
        self._check(self._lib.hf_set_materials(self._ctx, len(t), _pi(t), _pd(k), _pd(c)))

    def update_kappa(self, tags, kappa):
        """Overwrite the conductivity of some cell tags and re-assemble (kappa sweeps)."""
        t, k = _i32(tags), _f64(kappa)
        self._check(self._lib.hf_update_kappa(self._ctx, len(t), _pi(t), _pd(k)))

    def set_dirichlet(self, dofs):
        d = _i32(dofs)
        self._check(self._lib.hf_set_dirichlet(self._ctx, len(d), _pi(d) if len(d) else None))
        self._refresh_sizes()
        self._bc_dofs = d.copy()                # batch_get_operator sizes the lifting values by it

    def set_precond(self, kind=PC_JACOBI, reuse=False):
        """PC_JACOBI (0) or PC_AMG (1); call before assemble()."""
        self._check(self._lib.hf_set_precond(self._ctx, int(kind), 1 if reuse else 0))

    def set_time_scheme(self, scheme=TIME_BACKWARD_EULER):
        """TIME_BACKWARD_EULER (0, default) or TIME_BDF2 (1), or their names; call before assemble(), which keeps taking the
        real step.  A change invalidates the assembly and closes an open batch."""
        code = time_scheme_code(scheme) if isinstance(scheme, str) else int(scheme)
        self._check(self._lib.hf_set_time_scheme(self._ctx, code))

    def set_start_vector(self, kind=3):
        """0: u^n, 1: 2u^n - u^{n-1}, 2: that + response to the boundary values' second difference, 3 (default):
        A-norm projection on the last solutions and the boundary responses."""
        self._check(self._lib.hf_set_start_vector(self._ctx, int(kind)))

    def response_solves(self):
        c = C.c_int64()
        self._check(self._lib.hf_get_response_solves(self._ctx, C.byref(c)))
        return int(c.value)

    def amg_info(self):
        nl, opc, secs = C.c_int32(), C.c_double(), C.c_double()
        rows = np.zeros(16, dtype=np.int32)
        self._check(self._lib.hf_get_amg_info(self._ctx, C.byref(nl), _pi(rows), 16, C.byref(opc), C.byref(secs)))
        fb = C.c_int64()
        self._check(self._lib.hf_get_amg_fallbacks(self._ctx, C.byref(fb)))
        return {"levels": nl.value, "rows": rows[:nl.value].tolist(), "op_complexity": opc.value, "setup_s": secs.value,
                "jacobi_fallbacks": fb.value}

    def assemble(self, dt, mode=ASM_LDS_ATOMIC):
        self._check(self._lib.hf_assemble(self._ctx, float(dt), int(mode)))

    # -- state ---------------------------------------------------------------------------
    def set_state(self, u):
        u = _f64(u)
        if u.shape != (self.n,):
            raise ValueError(f"set_state: expected {self.n} values")
        self._check(self._lib.hf_set_state(self._ctx, _pd(u)))

    def get_state(self):
        u = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.hf_get_state(self._ctx, _pd(u)))
        return u

    def sample(self, nodes):
        idx = _i32(nodes)
        out = np.empty(len(idx), dtype=np.float64)
        self._check(self._lib.hf_sample(self._ctx, len(idx), _pi(idx), _pd(out)))
        return out

    # -- time stepping -------------------------------------------------------------------
    def step(self, g_bc, rtol=1e-10, atol=0.0, max_it=20000):
        g = _f64(g_bc)
        if g.shape != (self.n_bc,):
            raise ValueError(f"step: expected {self.n_bc} boundary values")
        it, res = C.c_int32(), C.c_double()
        rc = self._lib.hf_step(self._ctx, _pd(g) if self.n_bc else None, rtol, atol, int(max_it), C.byref(it), C.byref(res))
        self.last_iters, self.last_resid = it.value, res.value
        self._check(rc)
        return it.value, res.value

    def run(self, g_all, rtol=1e-10, atol=0.0, max_it=20000, nodes=None):
        g = _f64(g_all)
        if g.ndim != 2 or g.shape[1] != self.n_bc:
            raise ValueError(f"run: g_all must be (n_steps, {self.n_bc})")
        nsteps = g.shape[0]
        idx = _i32(nodes) if nodes is not None and len(nodes) else None
        ns = 0 if idx is None else len(idx)
        samples = np.empty((nsteps, ns), dtype=np.float64)
        iters = np.zeros(nsteps, dtype=np.int32)
        rc = self._lib.hf_run(self._ctx, nsteps, _pd(g) if self.n_bc else None, rtol, atol, int(max_it), ns, _pi(idx),
                              _pd(samples) if ns else None, _pi(iters))
        self.last_run_iters = iters
        self._check(rc)
        return samples, iters

    # -- variable time steps ----------------------------------------------------
    def set_step(self, dt):
        """The following steps of step / run have size ``dt`` (hf_set_step); the operator is re-valued by the next step whose
        effective step differs from the one it holds."""
        self._check(self._lib.hf_set_step(self._ctx, float(dt)))

    def set_step_list(self, dts):
        """The sizes of the next steps, one consumed per step (hf_set_step_list); an empty list clears it."""
        d = _f64(dts).ravel()
        self._check(self._lib.hf_set_step_list(self._ctx, len(d), _pd(d) if len(d) else None))

    def set_step_control(self, on=True):
        """Keep what :meth:`step_error` and :meth:`step_reject` need (hf_set_step_control); switched on at rest."""
        self._check(self._lib.hf_set_step_control(self._ctx, 1 if on else 0))

    def step_error(self, atol=1.0, rtol=0.0):
        """The local-error indicator of the step taken last, max over the free rows of |estimate| / (atol + rtol |u|)
        (hf_get_step_error)."""
        err = C.c_double()
        self._check(self._lib.hf_get_step_error(self._ctx, float(atol), float(rtol), C.byref(err)))
        return err.value

    def step_reject(self):
        """Undo the step taken last (hf_step_reject)."""
        self._check(self._lib.hf_step_reject(self._ctx))

    def step_info(self):
        """{"t", "dt_last", "dt_eff", "revaluations"} of the context's time record (hf_get_step_info)."""
        t, dl, de, rv = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self._check(self._lib.hf_get_step_info(self._ctx, C.byref(t), C.byref(dl), C.byref(de), C.byref(rv)))
        return {"t": t.value, "dt_last": dl.value, "dt_eff": de.value, "revaluations": int(rv.value)}

    # -- tangent runs: derivatives of the time loop with respect to conductivities and boundary parameters ----------
    def tangent_setup(self, n_par, tag_col):
        """``n_par`` tangent columns (1..16; the library pads them to nv = 2, 4, 8 or 16); ``tag_col`` = {cell tag: column}
        for the tags whose conductivity a column scales (other tags: none).  Every tangent starts at zero."""
        tab = np.full(self.tab_len, -1, dtype=np.int32)
        for t, j in dict(tag_col).items():
            if not 0 <= int(t) < self.tab_len:
                raise ValueError(f"tangent_setup: tag {t} is not a cell tag of the mesh")
            tab[int(t)] = int(j)
        self.tangent_nv = 0
        self._check(self._lib.hf_tangent_setup(self._ctx, int(n_par), _pi(tab)))
        self.tangent_nv = next(v for v in (2, 4, 8, 16) if v >= int(n_par))

    def tangent_setup_dir(self, n_par, k=None, r=None, z=None):
        """``n_par`` tangent columns as :meth:`tangent_setup`, in the directional conductivities (hf_tangent_setup_dir, DESIGN.md
        3.13): ``k`` = {cell tag: column} for the tags whose kappa a column is (both directions, the ratio of k_aniso kept),
        ``r`` / ``z`` = the same for the absolute k_r / k_z of a tag.  Isotropic and anisotropic tags alike."""
        tabs = []
        for name, m in (("k", k), ("r", r), ("z", z)):
            if not m:
                tabs.append(None)
                continue
            tab = np.full(self.tab_len, -1, dtype=np.int32)
            for t, j in dict(m).items():
                if not 0 <= int(t) < self.tab_len:
                    raise ValueError(f"tangent_setup_dir: tag {t} ({name}) is not a cell tag of the mesh")
                tab[int(t)] = int(j)
            tabs.append(tab)
        self.tangent_nv = 0
        self._check(self._lib.hf_tangent_setup_dir(self._ctx, int(n_par), *(None if t is None else _pi(t) for t in tabs)))
        self.tangent_nv = next(v for v in (2, 4, 8, 16) if v >= int(n_par))

    def tangent_set_shape(self, j, vz):
        """Column j of the tangent set-up in force becomes (also) a shape column: the nodes move along z with the nodal velocity
        ``vz`` (n values, dz_i / dtheta_j), the triangles stay (hf_tangent_set_shape).  ``None`` removes the
        column's shape part.  At most 4 columns; every tangent starts from zero again."""
        if vz is None:
            self._check(self._lib.hf_tangent_set_shape(self._ctx, int(j), None))
            return
        v = np.ascontiguousarray(vz, dtype=np.float64).reshape(-1)
        if v.size != self.n:
            raise ValueError(f"tangent_set_shape: {v.size} velocities for {self.n} nodes")
        self._check(self._lib.hf_tangent_set_shape(self._ctx, int(j), _pd(v)))

    def tangent_set_capacity(self, tag_col):
        """``tag_col`` = {cell tag: column}: the column carries the rho_c (J/m^3/K) of the tag (hf_tangent_set_capacity, DESIGN.md
        3.16); several tags may share a column, and the column may have conductivity entries and a shape velocity too.  An empty
        mapping (or None) removes the capacity columns.  Every tangent starts from zero again."""
        tag_col = dict(tag_col or {})
        if not tag_col:
            self._check(self._lib.hf_tangent_set_capacity(self._ctx, 0, None))
            return
        tab = np.full(self.tab_len, -1, dtype=np.int32)
        for t, j in tag_col.items():
            if not 0 <= int(t) < self.tab_len:
                raise ValueError(f"tangent_set_capacity: tag {t} is not a cell tag of the mesh")
            tab[int(t)] = int(j)
        self._check(self._lib.hf_tangent_set_capacity(self._ctx, self.tab_len, _pi(tab)))

    def table_derivatives(self, on=True):
        """Allow tangent runs under kappa(T) / rho_c(T) tables (hf_table_derivatives; lagged scheme, one Picard
        sweep).  Needs tables; set_kappa_tables, set_rhoc_tables and set_picard switch it off again.  A change drops the tangent
        set-up."""
        self._check(self._lib.hf_table_derivatives(self._ctx, 1 if on else 0))
        self.tangent_nv = 0

    def tangent_set_tables(self, kind, tables):
        """Derivative tables of the tangent set-up in force (hf_tangent_set_tables): ``kind`` 0 = conductivity,
        1 = rho_c (or "kappa" / "rhoc"); ``tables`` = {(column, cell tag): values}, d(knot value)/d(parameter of the column) at
        the knots of the tag's table of that kind.  An empty mapping (or None) clears the kind.  Every tangent starts from zero
        again."""
        kind = {"kappa": 0, "rhoc": 1}.get(kind, kind)
        items = sorted(((int(c), int(t)), np.asarray(v, dtype=np.float64).ravel()) for (c, t), v in (tables or {}).items())
        if not items:
            self._check(self._lib.hf_tangent_set_tables(self._ctx, int(kind), 0, None, None, None))
            return
        cols = _i32([c for (c, _), _ in items])
        tags = _i32([t for (_, t), _ in items])
        vals = _f64(np.concatenate([v for _, v in items]))
        self._check(self._lib.hf_tangent_set_tables(self._ctx, int(kind), len(items), _pi(cols), _pi(tags), _pd(vals)))

    def tangent_set_source(self, coef):
        """Source columns of the tangent set-up in force (hf_tangent_set_source): ``coef`` (n_steps, nv, 3) holds
        (c0, c1, c2) per step and column, and step k after the call adds c0 F1 + c1 G_f + c2 G_d to the column's load.  Needs a
        differentiable source (:meth:`source_derivatives`).  ``None`` (or no rows) removes the source columns.  A schedule like
        the amplitudes': the tangents are not reset."""
        if coef is None or len(coef) == 0:
            self._check(self._lib.hf_tangent_set_source(self._ctx, 0, None))
            return
        c = _f64(coef)
        nv = self.tangent_nv or 2     # (no set-up: the library reports it)
        if c.ndim != 3 or c.shape[1:] != (nv, 3):
            raise ValueError(f"tangent_set_source: coef must be (n_steps, {nv}, 3), got {c.shape}")
        self._check(self._lib.hf_tangent_set_source(self._ctx, c.shape[0], _pd(c)))

    def tangent_load(self, j):
        """Column j of the tangent loads F = -K_j u at the current state, by the set-up in force (hf_tangent_load; tests and
        diagnostics)."""
        F = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.hf_tangent_load(self._ctx, int(j), _pd(F)))
        return F

    def run_tangent(self, g_all, h_all=None, rtol=1e-10, atol=0.0, max_it=20000, nodes=None):
        """hf_run plus the tangents.  g_all (n_steps, n_bc); h_all (n_steps, n_bc, nv) or None (all zero).  Returns the
        primal samples (n_steps, n_s) and iterations (n_steps,), the tangent samples (n_steps, nv, n_s) and the tangent
        iterations (n_steps, nv)."""
        g = _f64(g_all)
        if g.ndim != 2 or g.shape[1] != self.n_bc:
            raise ValueError(f"run_tangent: g_all must be (n_steps, {self.n_bc})")
        nsteps, nv = g.shape[0], self.tangent_nv or 2     # (no set-up: the library reports it)
        h = None
        if h_all is not None:
            h = _f64(h_all)
            if h.shape != (nsteps, self.n_bc, nv):
                raise ValueError(f"run_tangent: h_all must be ({nsteps}, {self.n_bc}, {nv})")
        idx = _i32(nodes) if nodes is not None and len(nodes) else None
        ns = 0 if idx is None else len(idx)
        samples = np.empty((nsteps, ns), dtype=np.float64)
        tsamples = np.empty((nsteps, nv, ns), dtype=np.float64)
        iters = np.zeros(nsteps, dtype=np.int32)
        titers = np.zeros((nsteps, nv), dtype=np.int32)
        rc = self._lib.hf_run_tangent(self._ctx, nsteps, _pd(g) if self.n_bc else None, _pd(h) if (h is not None and self.n_bc) else None,
                                      rtol, atol, int(max_it), ns, _pi(idx), _pd(samples) if ns else None, _pi(iters),
                                      _pd(tsamples) if ns else None, _pi(titers))
        self.last_run_iters = iters
        self._check(rc)
        return samples, iters, tsamples, titers

    def get_tangent(self, j):
        s = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.hf_get_tangent(self._ctx, int(j), _pd(s)))
        return s

    # -- temperature-dependent conductivities (hf_set_kappa_tables) ---------------------
    def set_kappa_tables(self, tables, picard=1):
        """``tables`` = {cell tag: (T0, dT, values)}: kappa(T) piecewise linear on T0 + i dT, clamped outside; an empty dict
        clears them.  Every step then re-values A at u^n (BDF2: 2 u^n - u^{n-1}), with ``picard`` sweeps per step (1..8).
        Invalidates the assembly: set the state, then assemble()."""
        items = sorted((int(t), v) for t, v in (tables or {}).items())
        if not items:
            self._check(self._lib.hf_set_kappa_tables(self._ctx, 0, None, None, None, None, None, int(picard)))
            return
        tags = _i32([t for t, _ in items])
        t0 = _f64([float(v[0]) for _, v in items])
        dT = _f64([float(v[1]) for _, v in items])
        vals = [np.asarray(v[2], dtype=np.float64).ravel() for _, v in items]
        nk = _i32([len(v) for v in vals])
        allv = _f64(np.concatenate(vals))
        self._check(self._lib.hf_set_kappa_tables(self._ctx, len(tags), _pi(tags), _pd(t0), _pd(dT), _pi(nk), _pd(allv),
                                                  int(picard)))

    def set_rhoc_tables(self, tables):
        """``tables`` = {cell tag: (T0, dT, values of rho * cv)}: heat capacities of the shape and evaluation of a conductivity
        table (hf_set_rhoc_tables); an empty dict clears them.  Every evaluation then re-values M as well as A.
        The Picard count is the one of set_kappa_tables, or set_picard.  Invalidates the assembly: set the state, then assemble()."""
        items = sorted((int(t), v) for t, v in (tables or {}).items())
        if not items:
            self._check(self._lib.hf_set_rhoc_tables(self._ctx, 0, None, None, None, None, None))
            return
        tags = _i32([t for t, _ in items])
        t0 = _f64([float(v[0]) for _, v in items])
        dT = _f64([float(v[1]) for _, v in items])
        vals = [np.asarray(v[2], dtype=np.float64).ravel() for _, v in items]
        nk = _i32([len(v) for v in vals])
        allv = _f64(np.concatenate(vals))
        self._check(self._lib.hf_set_rhoc_tables(self._ctx, len(tags), _pi(tags), _pd(t0), _pd(dT), _pi(nk), _pd(allv)))

    # -- tables on anisotropic tags (hf_set_aniso_tables) -------------------------------
    def set_aniso_tables(self, on):
        """Allow (``on`` true) or refuse again kappa(T) / rho_c(T) tables together with anisotropic tags.  Off by default and
        after every set_mesh; switching off while both are set is refused."""
        self._check(self._lib.hf_set_aniso_tables(self._ctx, 1 if on else 0))

    # -- anisotropic conductivities (hf_set_anisotropy) ---------------------------------
    def set_anisotropy(self, multipliers):
        """``multipliers`` = {cell tag: (m_r, m_z)}: the tag conducts with k_r = m_r k along r and k_z = m_z k along z; tags
        not listed are isotropic and an empty dict clears everything.  Call after set_materials.  Invalidates the assembly, a
        steady set-up and a tangent set-up: assemble() again."""
        items = sorted((int(t), v) for t, v in (multipliers or {}).items())
        if not items:
            self._check(self._lib.hf_set_anisotropy(self._ctx, 0, None, None, None))
            return
        for t, v in items:
            if len(tuple(v)) != 2:
                raise ValueError(f"set_anisotropy: tag {t} needs a pair (m_r, m_z)")
        tags = _i32([t for t, _ in items])
        m_r = _f64([float(v[0]) for _, v in items])
        m_z = _f64([float(v[1]) for _, v in items])
        self._check(self._lib.hf_set_anisotropy(self._ctx, len(tags), _pi(tags), _pd(m_z), _pd(m_r)))

    def set_picard(self, sweeps):
        """Picard sweeps per step (1..8) while tables of either kind are set (hf_set_picard)."""
        self._check(self._lib.hf_set_picard(self._ctx, int(sweeps)))

    def picard_change(self):
        """max |u^{n+1,p} - u^{n+1,p-1}| of the last step's last Picard sweep (u^{n+1,0} = the evaluation state)."""
        d = C.c_double()
        self._check(self._lib.hf_get_picard_change(self._ctx, C.byref(d)))
        return float(d.value)

    # -- the enthalpy form of the capacity and the stored heat ---------------------------
    def set_capacity_form(self, form):
        """``form`` = "lagged" (the default) or "enthalpy" (hf_set_capacity_form): energy-conserving steps under capacity
        tables, backward Euler only.  Invalidates the assembly: set the state, then assemble()."""
        if form not in CAPACITY_FORMS:
            raise ValueError(f"set_capacity_form: unknown form {form!r} (expected one of {sorted(CAPACITY_FORMS)})")
        self._check(self._lib.hf_set_capacity_form(self._ctx, CAPACITY_FORMS[form]))

    def set_picard_control(self, tol=0.0, relax=1.0, max_sweeps=8):
        """Stop rule, relaxation and sweep cap (1..64) of the enthalpy form's iteration (hf_set_picard_control); ``tol`` = 0
        runs every sweep."""
        self._check(self._lib.hf_set_picard_control(self._ctx, float(tol), float(relax), int(max_sweeps)))

    def picard_history(self):
        """(sweeps, change): per step since the form was set or the history cleared, the sweeps used and the last change_k."""
        n = C.c_int32()
        self._check(self._lib.hf_get_picard_history(self._ctx, None, None, 0, C.byref(n)))
        sweeps, change = np.zeros(n.value, dtype=np.int32), np.zeros(n.value, dtype=np.float64)
        if n.value:
            self._check(self._lib.hf_get_picard_history(self._ctx, _pi(sweeps), _pd(change), n.value, C.byref(n)))
        return sweeps, change

    def clear_picard_history(self):
        self._check(self._lib.hf_clear_picard_history(self._ctx))

    def enthalpy_revalue(self, un, e):
        """M and A (get_csr) as one sweep of the enthalpy form values them at the pair (u^n, e) - a test window."""
        un, e = _f64(un), _f64(e)
        if un.shape != (self.n,) or e.shape != (self.n,):
            raise ValueError(f"enthalpy_revalue: two vectors of {self.n} values expected")
        self._check(self._lib.hf_enthalpy_revalue(self._ctx, _pd(un), _pd(e)))

    def stored_heat(self, T_ref):
        """Per cell tag sum_e vol_e (H_tag(Tw_e(u)) - H_tag(T_ref)) of the current state, in J per radian (tab_len values;
        hf_stored_heat)."""
        out = np.zeros(self.tab_len, dtype=np.float64)
        self._check(self._lib.hf_stored_heat(self._ctx, float(T_ref), _pd(out)))
        return out

    def set_heat_records(self, on, T_ref=0.0):
        """One stored-heat record per step of step / run from now on, measured from ``T_ref`` (hf_set_heat_records)."""
        self._check(self._lib.hf_set_heat_records(self._ctx, 1 if on else 0, float(T_ref)))

    def heat_count(self):
        n = C.c_int32()
        self._check(self._lib.hf_heat_count(self._ctx, C.byref(n)))
        return int(n.value)

    def get_heat(self, first=0, count=None):
        """Heat records [first, first + count) (count None: to the last), an array (count, tab_len)."""
        count = self.heat_count() - int(first) if count is None else int(count)
        out = np.zeros((max(count, 0), self.tab_len), dtype=np.float64)
        self._check(self._lib.hf_get_heat(self._ctx, int(first), count, _pd(out) if out.size else None))
        return out

    def clear_heat_records(self):
        self._check(self._lib.hf_clear_heat_records(self._ctx))

    # -- batched time loop: nv sweep points as the columns of one multi-vector PCG ------------------
    def batch_begin(self, nv, per_column_operator=False):
        """``per_column_operator``: BATCH_SHARED (False), BATCH_PER_COLUMN (True) or BATCH_AFFINE."""
        self.batch_nv = 0
        self._check(self._lib.hf_batch_begin(self._ctx, int(nv), int(per_column_operator)))
        self.batch_nv = int(nv)

    def batch_set_affine(self, tags, delta):
        """Operators A_j = A + delta[j] * dt K(unit conductivity on the cell tags ``tags``), A = the context's operator."""
        t, d = _i32(tags), _f64(delta)
        if d.shape != (self.batch_nv,):
            raise ValueError(f"batch_set_affine: {self.batch_nv} deltas expected")
        self._check(self._lib.hf_batch_set_affine(self._ctx, len(t), _pi(t), _pd(d)))

    def batch_load_column(self, j):
        """Copy the context's current (assembled, eliminated) operator into column j of the batch."""
        self._check(self._lib.hf_batch_load_column(self._ctx, int(j)))

    def batch_set_state(self, j, u):
        u = _f64(u)
        if u.shape != (self.n,):
            raise ValueError(f"batch_set_state: expected {self.n} values")
        self._check(self._lib.hf_batch_set_state(self._ctx, int(j), _pd(u)))

    def batch_get_state(self, j):
        u = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.hf_batch_get_state(self._ctx, int(j), _pd(u)))
        return u

    def batch_run(self, g_all, rtol=1e-10, atol=0.0, max_it=20000, nodes=None, flux_nodes=None, flux_components=2,
                  flux_rtol=None, flux_max_it=5000):
        """g_all: (n_steps, n_bc, nv).  Returns samples (n_steps, nv, n_s) and iters (n_steps, nv).
        With ``flux_nodes`` every step is followed by the read-flux projection of every column (flux_setup() first;
        ``flux_components``: 1 = d/dz, 2 = d/dr, 3 = both) and a third array is returned: the projected gradient at those
        nodes, (n_steps, n_comp, nv, len(flux_nodes)), z before r."""
        g = _f64(g_all)
        if g.ndim != 3 or g.shape[1] != self.n_bc or (self.batch_nv and g.shape[2] != self.batch_nv):
            raise ValueError(f"batch_run: g_all must be (n_steps, {self.n_bc}, {self.batch_nv or 'nv'})")
        nv = self.batch_nv or g.shape[2]        # no batch open on this side: the library reports it
        nsteps = g.shape[0]
        idx = _i32(nodes) if nodes is not None and len(nodes) else None
        ns = 0 if idx is None else len(idx)
        samples = np.empty((nsteps, nv, ns), dtype=np.float64)
        iters = np.zeros((nsteps, nv), dtype=np.int32)
        if flux_nodes is None:
            rc = self._lib.hf_batch_run(self._ctx, nsteps, _pd(g) if self.n_bc else None, rtol, atol, int(max_it), ns, _pi(idx),
                                        _pd(samples) if ns else None, _pi(iters))
            self.last_run_iters = iters
            self._check(rc)
            return samples, iters
        fidx = _i32(flux_nodes)
        comps = int(flux_components)
        ncomp = (comps & 1) + ((comps >> 1) & 1)
        flux = np.empty((nsteps, ncomp, nv, len(fidx)), dtype=np.float64)
        fit = np.zeros((nsteps, max(ncomp, 1)), dtype=np.int32)
        rc = self._lib.hf_batch_run_flux(self._ctx, nsteps, _pd(g) if self.n_bc else None, rtol, atol, int(max_it), ns, _pi(idx),
                                         _pd(samples) if ns else None, _pi(iters), comps, float(rtol if flux_rtol is None else flux_rtol),
                                         int(flux_max_it), len(fidx), _pi(fidx), _pd(flux), _pi(fit))
        self.last_run_iters, self.last_flux_iters = iters, fit
        self._check(rc)
        return samples, iters, flux

    def batch_end(self):
        self._check(self._lib.hf_batch_end(self._ctx))
        self.batch_nv = 0

    # -- batches under kappa(T) / rho_c(T) tables (hf_set_batch_tables) ----------------------------------------
    def set_batch_tables(self, on):
        """Allow (``on`` true) or refuse again batch_begin while tables are set.  Under the switch the batch opens with
        per-column operators only and every step re-values them on the GPU, each column at its own state.  Off by default and
        after every set_mesh; switching off closes an open batch under tables."""
        self._check(self._lib.hf_set_batch_tables(self._ctx, 1 if on else 0))

    def batch_set_column_kappa(self, j, tags, k):
        """Column j's constant conductivities of the cell tags ``tags`` (tags without a conductivity table); the default is the
        context's."""
        t, v = _i32(tags).ravel(), _f64(k).ravel()
        if t.shape != v.shape:
            raise ValueError("batch_set_column_kappa: one conductivity per tag expected")
        self._check(self._lib.hf_batch_set_column_kappa(self._ctx, int(j), len(t), _pi(t), _pd(v)))

    def batch_revalue(self, max_workgroups=0):
        """Re-value and eliminate every column's operators at the batch's current states, without stepping (a test window).
        ``max_workgroups`` > 0 caps the kernel's grid."""
        self._check(self._lib.hf_batch_revalue(self._ctx, int(max_workgroups)))

    def lift_slots(self):
        """CSR positions of the lifting values: the pattern entries (free row, Dirichlet column), ascending."""
        rowptr, colidx = self.get_csr(values=False)[:2]
        is_bc = np.zeros(self.n, dtype=bool)
        is_bc[np.asarray(getattr(self, "_bc_dofs", []), dtype=np.int64)] = True
        rows = np.repeat(np.arange(self.n), np.diff(rowptr))
        return np.nonzero(~is_bc[rows] & is_bc[colidx])[0]

    def batch_get_operator(self, j, want_M=False):
        """Column j of the open batch's per-column operator, de-interleaved: dict(A=(nnz,), dinv=(n,), lift=(n_lift,)) and, with
        ``want_M`` (capacity tables in the batch), M=(nnz,).  ``lift`` follows :meth:`lift_slots`."""
        out = {"A": np.empty(self.nnz), "dinv": np.empty(self.n), "lift": np.empty(len(self.lift_slots()))}
        if want_M:
            out["M"] = np.empty(self.nnz)
        self._check(self._lib.hf_batch_get_operator(self._ctx, int(j), _pd(out["A"]), _pd(out["dinv"]),
                                                    _pd(out["lift"]) if len(out["lift"]) else None, _pd(out.get("M"))))
        return out

    # -- a source and monitor records of the open batch -----------------------------------------------------
    def _batch_columns(self, name, v):
        """``v`` as nv values: a scalar for every column, or one per column."""
        a = _f64(v).ravel()
        nv = self.batch_nv or len(a)            # no batch open on this side: the library reports it
        if a.size == 1:
            a = np.full(nv, a[0], dtype=np.float64)
        if a.shape != (nv,):
            raise ValueError(f"batch_set_source: {name} must be a scalar or {nv} values")
        return np.ascontiguousarray(a)

    def batch_set_source(self, tags, fwhm=1.0, z0=0.0, depth=float("inf")):
        """The open batch's own source: column j gets the load of set_source(tags, fwhm[j], z0, depth[j]) (``fwhm`` and ``depth``: a
        scalar or one value per column).  An empty ``tags`` (or None) removes it.  It dies with batch_end."""
        t = _i32([] if tags is None else tags).ravel()
        if len(t) == 0:
            self._check(self._lib.hf_batch_set_source(self._ctx, 0, None, 0.0, None, None))
            return
        f, d = self._batch_columns("fwhm", fwhm), self._batch_columns("depth", depth)
        self._check(self._lib.hf_batch_set_source(self._ctx, len(t), _pi(t), float(z0), _pd(f), _pd(d)))

    def batch_get_source(self, j):
        """Column j of the batch's source: F1_j at unit amplitude (n values)."""
        F = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.hf_batch_get_source(self._ctx, int(j), _pd(F)))
        return F

    def batch_set_source_amplitudes(self, p):
        """p[n_steps, nv]: the amplitudes of the next steps of batch_run, one column per sweep point.  An empty table (or None)
        means amplitude 0 for every step."""
        p = _f64([] if p is None else p)
        if p.size == 0:
            self._check(self._lib.hf_batch_set_source_amplitudes(self._ctx, 0, None))
            return
        if p.ndim != 2 or (self.batch_nv and p.shape[1] != self.batch_nv):
            raise ValueError(f"batch_set_source_amplitudes: p must be (n_steps, {self.batch_nv or 'nv'})")
        self._check(self._lib.hf_batch_set_source_amplitudes(self._ctx, p.shape[0], _pd(p)))

    def batch_set_monitors(self, on=True):
        """Switch the open batch's monitor records on (one per step of batch_run from now on, under the table of set_monitors,
        which is set before batch_begin) or off (the batch's records are dropped)."""
        self._check(self._lib.hf_batch_set_monitors(self._ctx, 1 if on else 0))

    def batch_monitor_now(self):
        """The record of the batch's current state, [nv, tab_len, 7] (fields: MONITOR_FIELDS); nothing is recorded."""
        out = np.empty((max(self.batch_nv, 1), self.tab_len, 7), dtype=np.float64)
        self._check(self._lib.hf_batch_monitor_now(self._ctx, _pd(out)))
        return out

    def batch_monitor_count(self):
        c = C.c_int32()
        self._check(self._lib.hf_batch_monitor_count(self._ctx, C.byref(c)))
        return int(c.value)

    def batch_get_monitors(self, first=0, count=None):
        """Records ``first`` .. ``first + count - 1`` of the open batch (default: all from ``first``) as [records, nv, tab_len, 7]."""
        first = int(first)
        count = self.batch_monitor_count() - first if count is None else int(count)
        out = np.empty((max(count, 0), max(self.batch_nv, 1), self.tab_len, 7), dtype=np.float64)
        self._check(self._lib.hf_batch_get_monitors(self._ctx, first, count, _pd(out)))
        return out

    # -- read-flux projection (run_no_diamond) ----------------------------------------------
    def flux_setup(self):
        self._check(self._lib.hf_flux_setup(self._ctx))

    def flux_project(self, rtol=1e-10, max_it=5000, want_z=True, want_r=True):
        """(grad_z, grad_r) of the current state, L2-projected onto P1 with weight r."""
        gz = np.empty(self.n, dtype=np.float64) if want_z else None
        gr = np.empty(self.n, dtype=np.float64) if want_r else None
        it = np.zeros(2, dtype=np.int32)
        self._check(self._lib.hf_flux_project(self._ctx, rtol, int(max_it), _pd(gz), _pd(gr), _pi(it)))
        self.last_flux_iters = it
        return gz, gr

    def flux_solve(self, rtol=1e-10, max_it=5000, want_z=True, want_r=True):
        """Project the current state's gradient on the device only (no copy); returns the iteration counts."""
        it = np.zeros(2, dtype=np.int32)
        self._check(self._lib.hf_flux_solve(self._ctx, (1 if want_z else 0) | (2 if want_r else 0), rtol, int(max_it), _pi(it)))
        self.last_flux_iters = it
        return it

    def flux_sample(self, nodes, want_z=True, want_r=True):
        """(grad_z[nodes], grad_r[nodes]) of the last projection."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        gz = np.empty(len(nodes), dtype=np.float64) if want_z else None
        gr = np.empty(len(nodes), dtype=np.float64) if want_r else None
        self._check(self._lib.hf_flux_sample(self._ctx, len(nodes), _pi(nodes), _pd(gz), _pd(gr)))
        return gz, gr

    # -- steady state and loads (with_ir_steady.ipynb cells 17-23) ---------------------------
    def steady_setup(self, dofs, precond=PC_JACOBI):
        """Assemble the r-weighted stiffness K and eliminate the steady Dirichlet set ``dofs`` (its own, independent of
        set_dirichlet's); ``precond``: PC_JACOBI or PC_AMG (a hierarchy of its own).  An empty set raises ValueError."""
        d = _i32(dofs)
        self._check(self._lib.hf_steady_setup(self._ctx, len(d), _pi(d) if len(d) else None, int(precond)))
        self.n_steady = len(d)

    def steady_solve(self, g, use_load=False, rtol=1e-10, atol=0.0, max_it=20000):
        """K u = F on the free rows with u = g on the steady set (order of steady_setup's dofs); F = the load when
        ``use_load`` and one is set, else 0.  The answer becomes the state.  Returns (iterations, relative residual)."""
        g = _f64(g)
        if g.shape != (getattr(self, "n_steady", -1),):
            raise ValueError(f"steady_solve: expected {getattr(self, 'n_steady', 0)} boundary values (steady_setup first)")
        it, res = C.c_int32(), C.c_double()
        rc = self._lib.hf_steady_solve(self._ctx, _pd(g), 1 if use_load else 0, rtol, atol, int(max_it), C.byref(it), C.byref(res))
        self.last_iters, self.last_resid = it.value, res.value
        self._check(rc)
        return it.value, res.value

    def steady_picard_setup(self, dofs, precond=PC_JACOBI):
        """steady_setup for the steady state under kappa(T) / rho_c(T) tables (hf_steady_picard_setup): K is
        valued at the current state through the conductivity tables; with no table set it is steady_setup's K."""
        d = _i32(dofs)
        self._check(self._lib.hf_steady_picard_setup(self._ctx, len(d), _pi(d) if len(d) else None, int(precond)))
        self.n_steady = len(d)

    def steady_picard_solve(self, g, use_load=False, rtol=1e-10, atol=0.0, max_it=20000, picard_tol=1e-6, max_sweeps=50):
        """Picard iteration K(x_{k-1}) x_k = F on the free rows, x_k = g on the steady set, from the current state until
        max |x_k - x_{k-1}| <= picard_tol.  The answer becomes the state.  Returns {"sweeps", "iters" (per sweep), "change",
        "nl_resid"}, also kept as ``last_picard``; raises NotConverged when max_sweeps run out or a linear solve fails (the
        state is then the last iterate and ``last_picard`` is filled)."""
        g = _f64(g)
        if g.shape != (getattr(self, "n_steady", -1),):
            raise ValueError(f"steady_picard_solve: expected {getattr(self, 'n_steady', 0)} boundary values (steady_picard_setup first)")
        ms = int(max_sweeps)
        sw, chg, nl = C.c_int32(), C.c_double(), C.c_double()
        its = np.zeros(max(ms, 1), dtype=np.int32)
        rc = self._lib.hf_steady_picard_solve(self._ctx, _pd(g), 1 if use_load else 0, rtol, atol, int(max_it), float(picard_tol), ms,
                                              C.byref(sw), _pi(its), C.byref(chg), C.byref(nl))
        info = {"sweeps": sw.value, "iters": [int(v) for v in its[:sw.value]], "change": chg.value, "nl_resid": nl.value}
        self.last_picard = info
        self.last_iters, self.last_resid = sum(info["iters"]), nl.value
        self._check(rc)
        return info

    def set_load(self, F):
        """Load of the time step (b = M u^n + dt F): n values, or None to clear it."""
        if F is None:
            self._check(self._lib.hf_set_load(self._ctx, None))
            return
        F = _f64(F)
        if F.shape != (self.n,):
            raise ValueError(f"set_load: expected {self.n} values")
        self._check(self._lib.hf_set_load(self._ctx, _pd(F)))

    def hold_load(self):
        """Set the load that holds the current state: (K u)_i off the Dirichlet rows of set_dirichlet, 0 on them."""
        self._check(self._lib.hf_hold_load(self._ctx))

    def get_load(self):
        F = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.hf_get_load(self._ctx, _pd(F)))
        return F

    # -- volumetric source: laser power absorbed in some cell tags (hf_set_source) --------
    def set_source(self, tags, fwhm=1.0, z0=0.0, depth=float("inf")):
        """Source shape s = exp(-4 ln2 r^2 / fwhm^2) exp(-|z - z0| / depth) inside the elements of the cell tags ``tags``
        (depth = inf: uniform in z); its load F1 is formed on the device.  An empty ``tags`` (or None) clears the source."""
        t = _i32([] if tags is None else tags).ravel()
        if len(t) == 0:
            self._check(self._lib.hf_set_source(self._ctx, 0, None, 1.0, 0.0, float("inf")))
            return
        self._check(self._lib.hf_set_source(self._ctx, len(t), _pi(t), float(fwhm), float(z0), float(depth)))

    def get_source(self):
        """F1: the source's load at unit amplitude (n values)."""
        F = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.hf_get_source(self._ctx, _pd(F)))
        return F

    def source_derivatives(self, on=True):
        """Make the current source differentiable (hf_source_derivatives): forms dF1/dfwhm and dF1/ddepth on the
        device, after which the tangent calls accept the source.  ``on = False`` frees that again; set_source switches it off."""
        self._check(self._lib.hf_source_derivatives(self._ctx, 1 if on else 0))

    def get_source_derivative(self, which):
        """dF1/dfwhm (``which`` = 0 or "fwhm") or dF1/ddepth (1 or "depth") of a differentiable source (n values)."""
        w = {"fwhm": 0, "depth": 1}.get(which, which)
        G = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.hf_get_source_derivative(self._ctx, int(w), _pd(G)))
        return G

    def set_source_amplitudes(self, p):
        """Amplitudes (peak power densities, W/m^3) of the next len(p) steps: step k after the call uses p[k].  An empty list
        means amplitude 0 for every step."""
        p = _f64([] if p is None else p).ravel()
        self._check(self._lib.hf_set_source_amplitudes(self._ctx, len(p), _pd(p) if len(p) else None))

    # -- region monitors: per cell tag the extremes, int r dA, int u r dA and the hot part after every step ----
    MONITOR_FIELDS = ("T_max", "node_max", "T_min", "node_min", "I0", "I1", "H")

    def set_monitors(self, thresholds):
        """``thresholds`` = {cell tag: theta | None}: the tag is monitored, with the hot part H taken above ``theta`` (None, or
        +inf: no hot part, H = 0).  An empty mapping (or None) removes the monitors.  Every call drops the records."""
        thresholds = dict(thresholds or {})
        if not thresholds:
            self._check(self._lib.hf_set_monitors(self._ctx, 0, None))
            return
        tab = np.full(max(self.tab_len, max(int(t) for t in thresholds) + 1), np.nan, dtype=np.float64)
        for t, th in thresholds.items():
            if int(t) < 0:
                raise ValueError(f"set_monitors: tag {t} is not a cell tag of the mesh")
            th = float("inf") if th is None else float(th)
            if np.isnan(th):
                raise ValueError(f"set_monitors: the threshold of tag {t} is NaN (leave the tag out, or None for no hot part)")
            tab[int(t)] = th
        self._check(self._lib.hf_set_monitors(self._ctx, len(tab), _pd(tab)))

    def monitor_now(self):
        """The record of the current state, [tab_len, 7] (fields: MONITOR_FIELDS); nothing is recorded."""
        out = np.empty((self.tab_len, 7), dtype=np.float64)
        self._check(self._lib.hf_monitor_now(self._ctx, _pd(out)))
        return out

    def monitor_count(self):
        c = C.c_int32()
        self._check(self._lib.hf_monitor_count(self._ctx, C.byref(c)))
        return int(c.value)

    def get_monitors(self, first=0, count=None):
        """Records ``first`` .. ``first + count - 1`` (default: all from ``first``) as an array [records, tab_len, 7]: one per step of
        step / run / run_tangent since set_monitors / clear_monitor_records; rows of tags that are not monitored are zeros."""
        first = int(first)
        count = self.monitor_count() - first if count is None else int(count)
        out = np.empty((max(count, 0), self.tab_len, 7), dtype=np.float64)
        self._check(self._lib.hf_get_monitors(self._ctx, first, count, _pd(out)))
        return out

    def clear_monitor_records(self):
        """Drop the records; the table of monitored tags stays."""
        self._check(self._lib.hf_monitor_clear(self._ctx))

    # -- derivatives of the monitor sums along the tangent columns --------------------------------------------
    MONITOR_TANGENT_FIELDS = ("dT_max", "dT_min", "dI0", "dI1", "dH")

    def set_monitor_tangents(self, on):
        """Switch the derivative records of run_tangent on or off (monitors must be set to switch them on)."""
        self._check(self._lib.hf_set_monitor_tangents(self._ctx, 1 if on else 0))

    def monitor_tangent_count(self):
        """(derivative records kept, nv of their columns)."""
        c, nv = C.c_int32(), C.c_int32()
        self._check(self._lib.hf_monitor_tangent_count(self._ctx, C.byref(c), C.byref(nv)))
        return int(c.value), int(nv.value)

    def get_monitor_tangents(self, first=0, count=None):
        """Derivative records ``first`` .. ``first + count - 1`` (default: all from ``first``) as (array [K, tab_len, nv, 5] with the
        fields MONITOR_TANGENT_FIELDS, index [K] of the primal record of get_monitors each one belongs to)."""
        first = int(first)
        kept, nv = self.monitor_tangent_count()
        count = kept - first if count is None else int(count)
        out = np.empty((max(count, 0), self.tab_len, max(nv, 0), 5), dtype=np.float64)
        index = np.empty(max(count, 0), dtype=np.int32)
        self._check(self._lib.hf_get_monitor_tangents(self._ctx, first, count, _pd(out), _pi(index)))
        return out, index

    def monitor_tangent_eval(self, s, shape=None):
        """The derivative row [tab_len, nv, 5] of the current state for the tangent fields ``s`` [n, nv] (nv = 2, 4, 8 or 16) and
        ``shape`` = {column: nodal z-velocity} (at most 4): the kernels of the records on fields of the caller's; nothing is
        recorded, and the monitors of the current state are evaluated on the way."""
        s = np.ascontiguousarray(s, dtype=np.float64)
        if s.ndim != 2 or s.shape[0] != self.n:
            raise ValueError(f"monitor_tangent_eval: s must be [n = {self.n}, nv] (got {s.shape})")
        shape = dict(shape or {})
        cols = np.array(list(shape), dtype=np.int32)
        vz = np.zeros((self.n, len(cols)), dtype=np.float64)
        for q, j in enumerate(shape):
            v = np.asarray(shape[j], dtype=np.float64).ravel()
            if v.size != self.n:
                raise ValueError(f"monitor_tangent_eval: shape column {j}: {self.n} velocities expected (got {v.size})")
            vz[:, q] = v
        out = np.empty((self.tab_len, s.shape[1], 5), dtype=np.float64)
        self._check(self._lib.hf_monitor_tangent_eval(self._ctx, s.shape[1], _pd(s), len(cols), _pi(cols) if len(cols) else None,
                                                      _pd(vz) if len(cols) else None, _pd(out)))
        return out

    # -- inspection ----------------------------------------------------------------------
    def get_csr(self, values=True):
        rowptr = np.empty(self.n + 1, dtype=np.int32)
        colidx = np.empty(self.nnz, dtype=np.int32)
        A = np.empty(self.nnz, dtype=np.float64) if values else None
        M = np.empty(self.nnz, dtype=np.float64) if values else None
        self._check(self._lib.hf_get_csr(self._ctx, _pi(rowptr), _pi(colidx), _pd(A), _pd(M)))
        return rowptr, colidx, A, M

    def spmv(self, x, which=0):
        x = _f64(x)
        y = np.empty(self.n, dtype=np.float64)
        self._check(self._lib.hf_spmv(self._ctx, int(which), _pd(x), _pd(y)))
        return y

    def set_value_lists(self, mode):
        """Value lists of A and M for the fine-level SpMV (0 off, 1 where they hold <= nnz / 2 entries, 2 always); effective
        from the next assemble."""
        self._check(self._lib.hf_set_value_lists(self._ctx, int(mode)))

    def get_value_lists(self, which=0, arrays=False):
        """dict(valid, sum_vlist, max_vlist, vcap) of the value lists of A (which = 0) or M (1); with arrays=True also vptr,
        vlist and cv (the tables must be valid)."""
        valid, mx, vcap, total = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._lib.hf_get_value_lists(self._ctx, int(which), C.byref(valid), C.byref(total), C.byref(mx), C.byref(vcap),
                                                 None, None, None))
        out = {"valid": bool(valid.value), "sum_vlist": total.value, "max_vlist": mx.value, "vcap": vcap.value}
        if arrays:
            vptr = np.empty((self.n + 511) // 512 + 1, dtype=np.int32)
            vlist = np.empty(total.value, dtype=np.float64)
            cv = np.empty(self.nnz, dtype=np.uint32)
            self._check(self._lib.hf_get_value_lists(self._ctx, int(which), None, None, None, None, _pi(vptr), _pd(vlist),
                                                     cv.ctypes.data_as(C.POINTER(C.c_uint32))))
            out.update(vptr=vptr, vlist=vlist, cv=cv)
        return out

    # -- start-vector test entry point (tests/test_gpu_start_vector.py) ---------------------------------
    def projection_sizes(self):
        return projection_sizes()

    def get_projection(self, column=-1, arrays=False):
        """The projection basis of the start vector (kind 3): dict(mh, mt, used (mt bools), next, pending, G (mt, mt) by slot,
        alpha (mt coefficients by slot), rank); with arrays=True also V and F (mt, n), zero rows for slots not in use.
        column = -1: the basis of step() / run(); column = j: column j of the open batch."""
        mh, mt = self.projection_sizes()
        used = np.zeros(mt, dtype=np.int32)
        nxt, pend = C.c_int32(), C.c_int32()
        G, alpha = np.empty((mt, mt)), np.empty(mt + 1)
        V = np.empty((mt, self.n)) if arrays else None
        F = np.empty((mt, self.n)) if arrays else None
        self._check(self._lib.hf_get_projection(self._ctx, int(column), None, None, _pi(used), C.byref(nxt), C.byref(pend), _pd(G),
                                                _pd(alpha), _pd(V), _pd(F)))
        out = {"mh": mh, "mt": mt, "used": used.astype(bool), "next": nxt.value, "pending": pend.value, "G": G, "alpha": alpha[:mt].copy(),
               "rank": int(alpha[mt])}                                        # (zero until the first solve: the buffer is cleared when allocated)
        if arrays:
            out.update(V=V, F=F)
        return out

    # -- read-flux test entry point (tests/test_gpu_flux.py) ---------------------------------------------
    def flux_system(self, column=-1, matrix=False, want_z=True, want_r=True):
        """The linear systems of the read-flux projection: dict(bz, br) - the right-hand sides the last flux_solve /
        flux_project formed (column = -1), or column j of the open batch's projection, which holds one component at a time
        (ask for that one alone); a component not asked for is None.  matrix=True adds M1 (nnz values on get_csr's pattern)
        and dinv1 (n)."""
        M1 = np.empty(self.nnz, dtype=np.float64) if matrix else None
        dinv1 = np.empty(self.n, dtype=np.float64) if matrix else None
        bz = np.empty(self.n, dtype=np.float64) if want_z else None
        br = np.empty(self.n, dtype=np.float64) if want_r else None
        self._check(self._lib.hf_get_flux_system(self._ctx, int(column), _pd(M1), _pd(dinv1), _pd(bz), _pd(br)))
        out = {"bz": bz, "br": br}
        if matrix:
            out.update(M1=M1, dinv1=dinv1)
        return out

    # -- preconditioner test entry points (tests/test_gpu_vcycle.py) ------------------------------------
    def amg_apply(self, r):
        """(z, rz): z = B r, one V-cycle as the single-run PCG applies it, and the r.z sum it leaves for PCG."""
        r = _f64(r)
        if r.shape != (self.n,):
            raise ValueError(f"amg_apply: vector of {self.n} entries expected")
        z = np.empty(self.n, dtype=np.float64)
        rz = C.c_double()
        self._check(self._lib.hf_amg_apply(self._ctx, _pd(r), _pd(z), C.byref(rz)))
        return z, rz.value

    def batch_apply_precond(self, R):
        """(Z, rz): the batched V-cycle of the open batch on the columns R[j] (shape (nv, n)), and the nv r.z values."""
        R = _f64(R)
        if R.shape != (self.batch_nv, self.n):
            raise ValueError(f"batch_apply_precond: array of shape ({self.batch_nv}, {self.n}) expected")
        Z = np.empty_like(R)
        rz = np.empty(self.batch_nv, dtype=np.float64)
        self._check(self._lib.hf_batch_apply_precond(self._ctx, _pd(R), _pd(Z), _pd(rz)))
        return Z, rz

    def dense_inverse(self, S, b):
        """(inv, x64, x32) of the coarsest level's dense solve on the SPD scipy sparse matrix S: the f64 inverse formed on
        the device, inv @ b through the f64 dense mat-vec, and through the f32 one on float(inv)."""
        S = S.tocsr()
        S.sort_indices()
        n = S.shape[0]
        ptr, idx, val, b = _i32(S.indptr), _i32(S.indices), _f64(S.data), _f64(b)
        inv = np.empty((n, n), dtype=np.float64)
        x64 = np.empty(n, dtype=np.float64)
        x32 = np.empty(n, dtype=np.float64)
        self._check(self._lib.hf_dense_inverse(self._ctx, int(n), _pi(ptr), _pi(idx), _pd(val), _pd(b), _pd(inv), _pd(x64), _pd(x32)))
        return inv, x64, x32

    def time_kernel(self, which, reps=50):
        ms = C.c_double()
        self._check(self._lib.hf_time_kernel(self._ctx, int(which), int(reps), C.byref(ms)))
        return ms.value

    def set_profile(self, on=True):
        self._check(self._lib.hf_set_profile(self._ctx, 1 if on else 0))

    def get_profile(self):
        """(summed ms, launches) of the PCG SpMV launches bracketed since set_profile(True)."""
        ms, cnt = C.c_double(), C.c_int64()
        self._check(self._lib.hf_get_profile(self._ctx, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def last_gpu_ms(self):
        ms = C.c_double()
        self._check(self._lib.hf_last_gpu_ms(self._ctx, C.byref(ms)))
        return ms.value

    @staticmethod
    def version():
        return load_library().hf_version().decode()
