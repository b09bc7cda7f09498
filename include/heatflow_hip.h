/*
 * heatflow_hip.h - C ABI of libheatflow_hip.so (MI355X / gfx950, HIP).
 *
 * Drop-in boundary for the hot path of cebarker1000/heatflow.  The reference has no
 * FFI layer: its drivers call dolfinx / PETSc directly from Python.  Each entry point
 * below names the reference call(s) it stands in for (file:line in the reference):
 *
 *   hf_set_mesh        gmshio.model_to_mesh(...)            run_with_diamond.py:240-245
 *                      fem.functionspace(domain, P1 / DG0)  run_with_diamond.py:279-280
 *   hf_set_mesh_prebuilt / hf_pattern_export   the same for the 2nd..Nth worker of a sweep, which in the
 *                      reference re-reads mesh.msh and rebuilds everything   parameter_sweep.py:401-446
 *   hf_set_materials   kappa.x.array[:] / rho_cv.x.array[:] run_with_diamond.py:286-301
 *   hf_set_dirichlet   fem.dirichletbc(g, row_dofs) x 4     dirichlet_bc/bc.py:104-113,
 *                                                           run_with_diamond.py:362-374
 *   hf_assemble        fem.form(lhs) + assemble_matrix(lhs_form, bcs) + KSP/PC setup
 *                                                           run_with_diamond.py:328-337, 381-394
 *   hf_set_state       u_n.x.array[:] = ic_temp             run_with_diamond.py:317-319
 *   hf_step            b.set(0); assemble_vector(b, rhs_form); apply_lifting; ghostUpdate;
 *                      set_bc; solver.solve(b, u_n)         run_with_diamond.py:474-481
 *   hf_sample          u_n.x.array[node_idx]                run_with_diamond.py:485-493
 *   hf_get_state       u_n.x.array (what xdmf.write_function would write)   :483-484
 *   hf_flux_setup      assemble_matrix(a_proj) + KSP/LU set-up       run_no_diamond.py:471-491
 *   hf_flux_project    assemble_vector(rhs_proj) + solver_proj.solve run_no_diamond.py:543-550
 *   hf_get_flux_system no counterpart: a test window on the projection's matrix and right-hand sides (see below)
 *   hf_steady_setup    Space.build_steady_state_variational_forms + assemble_matrix(a_ss, bcs_ss) + solver set-up
 *                                                           space/space_and_forms.py:119-149, with_ir_steady.ipynb cell 17
 *   hf_steady_solve    assemble_vector(L_ss) + apply_lifting + set_bc + solve     with_ir_steady.ipynb cell 17
 *   hf_set_load        the load term dt * f * v * r * dx of build_variational_forms  space/space_and_forms.py:77-117;
 *                      b_equiv uploaded as it stands                    with_ir_steady.ipynb cells 18, 22
 *   hf_hold_load       b_equiv = A_free . u_ss with the transient's Dirichlet rows zeroed   with_ir_steady.ipynb cell 18
 *   hf_set_time_scheme no counterpart: the reference steps with backward Euler only (run_with_diamond.py:321-337);
 *                      HF_TIME_BDF2 is the second-order alternative
 *   hf_tangent_setup / hf_tangent_setup_dir / hf_tangent_set_shape / hf_run_tangent / hf_get_tangent / hf_tangent_load   no counterpart: the reference fits by re-running the forward model
 *                      over a grid (sweep_test.py:47-75, parameter_sweep.py:195-235); these give the derivatives of a run
 *   hf_set_kappa_tables / hf_get_picard_change   no counterpart: the reference's conductivities are constants per material
 *                      (run_with_diamond.py:286-301); these make them functions of the temperature
 *   hf_set_rhoc_tables / hf_set_picard   no counterpart: the same for the heat capacity rho * cv (run_with_diamond.py:286-301)
 *   hf_set_anisotropy  no counterpart: the reference's conductivities are scalars (run_with_diamond.py:286-301); this makes
 *                      them diagonal tensors in (z, r)
 *
 * Conventions
 *   - All functions return 0 (HF_OK) or a negative HF_ERR_* code; hf_last_error(ctx)
 *     returns a message for the last failure on that context.
 *   - Host pointers are borrowed for the duration of the call only and copied to the
 *     device; outputs go to caller-allocated host buffers.  No torch / numpy types.
 *   - float64 values, int32 indices.  Node coordinates are (z, r) pairs: mesh x = z
 *     (axial), mesh y = r (radial), weight r = x[1] as in run_with_diamond.py:321-322.
 *   - One ctx = one HIP device + one stream.  A ctx is not thread-safe; different
 *     ctxs may be driven from different threads or processes (one per GPU).
 *   - hf_step / hf_run / hf_batch_run block until their steps are done; meanwhile the calling
 *     thread polls pinned host memory that the solver kernels update (no other thread is
 *     created).  No progress for HEATFLOW_POLL_TIMEOUT_S seconds (default 60) -> HF_ERR_HIP.
 *   - There is no CPU fallback: without a HIP device hf_create fails.
 */
#ifndef HEATFLOW_HIP_H
#define HEATFLOW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hf_ctx hf_ctx;

enum {
  HF_OK = 0,
  HF_ERR_ARG = -1,      /* bad argument (null pointer, index out of range, ...) */
  HF_ERR_STATE = -2,    /* call out of order (e.g. hf_step before hf_assemble) */
  HF_ERR_HIP = -3,      /* a HIP runtime call failed; see hf_last_error */
  HF_ERR_NOCONV = -4,   /* PCG hit max_it (or broke down) before reaching the tolerance */
  HF_ERR_ALLOC = -5
};

/* Assembly variants (all are per-element kernels, results agree to rounding):
 *   HF_ASM_LDS_ATOMIC    a workgroup owns 256 CSR rows, stages their value slab in LDS,
 *                        scatter-adds the incident elements with LDS f64 atomics and
 *                        streams the slab out once (coalesced).
 *   HF_ASM_LDS_COLORED   same staging, elements processed colour by colour with plain
 *                        LDS read-modify-write: bitwise reproducible.
 *   HF_ASM_GLOBAL_ATOMIC one thread per element, f64 atomics straight into global CSR
 *                        (baseline / cross-check).
 *   HF_ASM_ROW_GATHER    a lane owns one CSR row and visits the triangles at its node (16-bit
 *                        list entries = positions of the two other vertices in the row); the
 *                        slab, the column positions and the coordinates of the block live in
 *                        LDS, every global access is a coalesced stream; no atomics, no
 *                        colours, bitwise reproducible.  Default of the entry points.  Falls
 *                        back to HF_ASM_LDS_COLORED for meshes with a row of more than 32
 *                        entries or more than 64 distinct cell tags. */
enum { HF_ASM_LDS_ATOMIC = 0, HF_ASM_LDS_COLORED = 1, HF_ASM_GLOBAL_ATOMIC = 2, HF_ASM_ROW_GATHER = 3 };

/* Kernels addressable by hf_time_kernel */
enum {
  HF_K_SPMV = 0,        /* y = A x, CSR, LDS-staged products            */
  HF_K_PCG_SPMV = 1,    /* PCG iteration head: beta, Ap <- A z + beta Ap, p <- z + beta p, p.Ap partials */
  HF_K_PCG_UPDATE = 2,  /* x += a p; r -= a Ap; z = D^-1 r; r.z, z.z    */
  HF_K_PCG_DIR = 3,     /* retired: the direction update is fused into HF_K_PCG_SPMV (returns HF_ERR_ARG) */
  HF_K_ASSEMBLE = 4,    /* element kernel in the mode of the last hf_assemble */
  HF_K_RHS = 5,         /* b = M u^n                                    */
  HF_K_STREAM_READ = 6  /* plain streaming read of the operator's values + column indices (12 nnz bytes, 16-byte loads):
                           the read bandwidth this device reaches on the SpMV's own arrays - its practical ceiling */
};

const char* hf_version(void);

int hf_create(int device_id, hf_ctx** out);
int hf_destroy(hf_ctx* ctx);
const char* hf_last_error(const hf_ctx* ctx);

/* Mesh: n nodes, n_e P1 triangles.  zr = n x 2 (z, r); tri = n_e x 3 node ids;
 * tag = n_e cell tags (>= 0).  Builds the CSR sparsity pattern and the row-block
 * element lists once (host side) and uploads everything. */
int hf_set_mesh(hf_ctx* ctx, int32_t n, int32_t n_e, const double* zr, const int32_t* tri, const int32_t* tag);

/* The tables hf_set_mesh derives from the connectivity (CSR pattern, compressed column lists of the SpMV chunks,
 * row-gather assembly lists) in serialised form, so that ONE context builds them and every other context on the
 * same mesh - other ranks of a sweep, further contexts of the same rank - installs them without rebuilding:
 * the MI355X counterpart of the reference's workers each re-reading mesh.msh (parameter_sweep.py:401-446).
 * hf_pattern_export writes exactly hf_pattern_export_size bytes; hf_set_mesh_prebuilt = hf_set_mesh with the
 * tables taken from such a blob (validated against n, n_e and its own index ranges; the mesh arrays themselves
 * are trusted to be the ones the blob was exported for).  `blob` may be a host or a device pointer in both calls
 * (hipMemcpyDefault), so an RCCL broadcast buffer can be handed over as it is. */
int hf_pattern_export_size(hf_ctx* ctx, int64_t* bytes);
int hf_pattern_export(hf_ctx* ctx, void* blob, int64_t bytes);
int hf_set_mesh_prebuilt(hf_ctx* ctx, int32_t n, int32_t n_e, const double* zr, const int32_t* tri, const int32_t* tag,
                         const void* blob, int64_t bytes);

/* Cell-tag -> coefficient tables: kappa[c] = kappa[i], rho_c[c] = rho_c[i] for cells with
 * tag == tags[i].  May be called again (kappa sweep) followed by hf_assemble. */
int hf_set_materials(hf_ctx* ctx, int32_t n_mat, const int32_t* tags, const double* kappa, const double* rho_c);

/* Kappa sweep step: overwrite the conductivity of the listed cell tags (rho_c, mesh, pattern, Dirichlet
 * set, dt and assembly mode stay) and re-value M, A, D^-1 - i.e. hf_set_materials + hf_assemble for the
 * entries that changed (reference: a new run_simulation per kappa, sweep_test.py:55-75). */
int hf_update_kappa(hf_ctx* ctx, int32_t n_mat, const int32_t* tags, const double* kappa);

/* Anisotropic conductivities: cells with tag == tags[i] conduct with k_z = m_z[i] * kappa along z and k_r = m_r[i] * kappa along
 * r (kappa from hf_set_materials / hf_update_kappa, which scale both directions: the ratio stays).  The tensor is diagonal in
 * (z, r) and constant per element; M does not change.  Unlisted tags are isotropic, a listed tag with both multipliers 1 counts
 * as isotropic, n = 0 clears.  While no tag is anisotropic the existing kernels run and nothing changes; otherwise the row-gather
 * kernel k_assemble_rows_an assembles M, A (hf_assemble, hf_update_kappa), the stiffness of hf_steady_setup (hence hf_hold_load)
 * and the A1 of hf_batch_set_affine; everything above the assembly reads M and A only and works unchanged.
 * Call after hf_set_materials (it stays over later hf_set_materials calls; hf_set_mesh clears it).  A call that changes anything
 * invalidates the assembly, a steady set-up and a tangent set-up, and closes an open batch: hf_assemble (hf_steady_setup,
 * hf_tangent_setup) again.  The multipliers belong to the multigrid fingerprint: a hierarchy kept under hf_set_precond(1, reuse = 1)
 * or installed by hf_amg_install meets an operator with other multipliers as a frozen one.
 * Errors: HF_ERR_STATE before hf_set_materials, and, for a call that leaves a tag anisotropic, while kappa(T) / rho_c(T) tables
 * are set (the table kernels are isotropic);
 * HF_ERR_ARG for a tag that is not a cell tag of the mesh, a tag listed twice, a multiplier that is not finite and positive, and
 * on a mesh without row-gather lists or after hf_assemble in another mode.  While a tag is anisotropic: hf_assemble in a mode
 * other than HF_ASM_ROW_GATHER -> HF_ERR_ARG; hf_set_kappa_tables, hf_set_rhoc_tables and hf_steady_picard_setup -> HF_ERR_STATE;
 * hf_tangent_setup with a column on an anisotropic tag -> HF_ERR_ARG (columns on isotropic tags work: their load is the unit
 * stiffness of those tags and the operator is the primal's).  hf_tangent_setup_dir takes columns in k_r, k_z and kappa of any
 * tag, anisotropic ones included; the derivative with respect to a multiplier is kappa times the directional one. */
int hf_set_anisotropy(hf_ctx* ctx, int32_t n, const int32_t* tags, const double* m_z, const double* m_r);

/* Tables on anisotropic tags (opt-in).  Off by default, and hf_set_mesh switches it off: every call, message
 * and error code is then the one documented above.  on != 0 lifts four of the refusals: hf_set_kappa_tables, hf_set_rhoc_tables
 * and hf_steady_picard_setup are accepted while a tag is anisotropic, and hf_set_anisotropy while tables are set.  A tag keeps
 * its multipliers and its scalar conductivity is table(T_e) where it has a table, else its constant:
 *     k_r = m_r kappa(T_e),  k_z = m_z kappa(T_e)   (the ratio does not depend on the temperature),  rho_c(T_e) as without multipliers,
 * with T_e the element temperature of hf_set_kappa_tables.  While tables and an anisotropic tag are both set, the re-valuations
 * run k_assemble_rows_kT_an / k_assemble_rows_cT_an (the time step, hf_assemble) and k_assemble_rows_kT_K_an (the Picard steady
 * state) in place of their isotropic siblings; otherwise nothing new is launched.  With every multiplier 1 the results are the
 * isotropic table path's bit for bit, with constant tables those of hf_set_anisotropy alone.  The staleness rules of both calls
 * stay as they are.
 * Still refused under the switch (HF_ERR_STATE, the message names the call): hf_table_derivatives(1) and hf_tangent_set_tables
 * while a tag is anisotropic; hf_set_anisotropy leaving a tag anisotropic while table derivatives are on; hf_tangent_setup,
 * hf_tangent_setup_dir and hf_run_tangent while tables are set on an anisotropic context (the table loads and the directional
 * loads know nothing of each other); hf_batch_begin under tables; and (HF_ERR_ARG) every assembly mode but HF_ASM_ROW_GATHER.
 * Errors: HF_ERR_STATE before hf_set_mesh, and for on == 0 while tables and an anisotropic tag are both set (the message names
 * both: clear one first). */
int hf_set_aniso_tables(hf_ctx* ctx, int32_t on);

/* Dirichlet DOFs (unique; the host resolves overlaps "later BC wins" beforehand).
 * The order defines the order of g_bc in hf_step.  n_bc = 0 removes all BCs. */
int hf_set_dirichlet(hf_ctx* ctx, int32_t n_bc, const int32_t* dofs);

/* M = M_r(rho_c), A = M + dt K_r(kappa); then rows+columns of the Dirichlet DOFs are
 * zeroed with unit diagonal (the lifting columns are kept aside) and D^-1 is formed. */
int hf_assemble(hf_ctx* ctx, double dt, int32_t mode);

/* Time scheme of every transient loop (hf_step, hf_run, the batched loop, tangent runs):
 *   HF_TIME_BACKWARD_EULER (default)  A u^{n+1} = M u^n + dt F,                       A = M + dt K
 *   HF_TIME_BDF2                      A' u^{n+1} = M (4/3 u^n - 1/3 u^{n-1}) + dt' F,  A' = M + dt' K, dt' = 2 dt / 3
 *                                     (the constant-step BDF2 formula (3/2 M + dt K) u^{n+1} = 2 M u^n - 1/2 M u^{n-1} + dt F
 *                                     divided by 3/2; lifting and set_bc as before, with A').
 * Call before hf_assemble, which keeps taking the real step dt and, under BDF2, assembles A' - so hf_get_csr / hf_spmv then
 * return A' = M + (2/3) dt K (Dirichlet-eliminated), hf_update_kappa / hf_batch_set_affine re-value A' and the affine part is
 * dt' K.  A change of scheme invalidates the assembly (hf_step, hf_run, hf_batch_begin / hf_batch_run, hf_run_tangent return
 * HF_ERR_STATE until the next hf_assemble) and closes an open batch; setting the current scheme again changes nothing.  The
 * multigrid fingerprint includes the scheme: a hierarchy built for one scheme meets the other's operator as a frozen one.
 * History: u^{n-1} is kept under BDF2 whatever the start-vector kind.  hf_set_state, hf_steady_solve, hf_assemble (hence
 * hf_update_kappa), hf_batch_begin and hf_tangent_setup / the tangent resets start it at rest, u^{-1} = u^n (s^{-1} = s^0 = 0
 * for tangents): exact for a uniform initial state and for a held steady state.  hf_batch_set_state(j) sets column j's
 * history to its new state.  A second hf_run / hf_batch_run / hf_run_tangent continues with the true u^{n-1}.
 * Start vectors under BDF2: kinds 0, 1 and 3 as documented; kind 2's response correction assumes the one-step recursion of
 * backward Euler and is not used - kind 2 runs as kind 1.  The boundary responses stay in kind 3's projection basis.
 * HF_ERR_ARG for an unknown scheme. */
enum { HF_TIME_BACKWARD_EULER = 0, HF_TIME_BDF2 = 1 };
int hf_set_time_scheme(hf_ctx* ctx, int32_t scheme);

/* Preconditioner of the PCG solve: kind 0 = Jacobi (D^-1, the north-star path), kind 1 =
 * smoothed-aggregation multigrid V(1,1) with damped-Jacobi smoothing, built on the host from the
 * assembled operator at hf_assemble time and applied on the GPU with CSR SpMV kernels.  With
 * reuse != 0 the coarse levels are kept across later hf_assemble calls (kappa sweeps on one mesh:
 * the fine level always uses the current matrix, the frozen coarse levels remain a valid SPD
 * preconditioner).  Call before hf_assemble.  The stopping criterion of hf_step is the same for both. */
int hf_set_precond(hf_ctx* ctx, int32_t kind, int32_t reuse);
/* Hierarchy of the last AMG set-up: level count, rows per level (up to max_levels entries),
 * operator complexity sum(nnz_l)/nnz_0 and host set-up time.  Any pointer may be NULL. */
int hf_get_amg_info(hf_ctx* ctx, int32_t* n_levels, int32_t* level_rows, int32_t max_levels, double* op_complexity,
                    double* setup_seconds);

/* The hierarchy of a context as one blob, for other contexts on the same mesh (the other sessions of a sweep, on this
 * GPU or - broadcast with the mesh - on the other ranks): what the host set-up computes is shipped instead of recomputed.
 * The reference's analogue is the per-worker MUMPS factorisation (run_with_diamond.py:389-394; every pool worker of
 * parameter_sweep.py:401-446 factorises for itself).  hf_amg_export needs a completed hf_assemble with the multigrid
 * preconditioner; blob = host or device memory of hf_amg_export_size bytes.  hf_amg_install needs hf_set_mesh,
 * hf_set_dirichlet and hf_set_precond(1, reuse = 1) on the same mesh and is followed by hf_assemble, which keeps the
 * installed hierarchy instead of building one and compares its own operator with the fingerprint in the blob (time step,
 * coefficient tables, hf_set_anisotropy's multipliers, Dirichlet set): the same operator -> the cycle is the one the exporting context runs, bit for bit;
 * another point of a sweep -> the hierarchy is a frozen one (see hf_set_precond).  Every index in the blob is
 * verified; HF_ERR_ARG if it does not belong to this mesh. */
int hf_amg_export_size(hf_ctx* ctx, int64_t* bytes);
int hf_amg_export(hf_ctx* ctx, void* blob, int64_t bytes);
int hf_amg_install(hf_ctx* ctx, const void* blob, int64_t bytes);

/* Start vector of every hf_step / hf_run solve (the converged answer does not depend on it, only the
 * iteration count does): kind 0 = u^n (what KSP.solve sees in the reference, run_with_diamond.py:480,
 * where it is irrelevant because the solve is direct); 1 = 2 u^n - u^{n-1}; 2 = that plus the
 * response to the second difference of the boundary values: the loop is linear,
 * u^{n+1} = T u^n + R g^{n+1}, so  u^{n+1} - 2u^n + u^{n-1} = T(...) + R (g^{n+1} - 2g^n + g^{n-1});  R d is
 * obtained by one extra solve the first time a new direction d of that second difference appears (the
 * heated line's Gaussian profile: once per assembled operator) and re-used, scaled, afterwards;
 * 3 (default) = Galerkin projection: the combination of the last six solutions and of those boundary responses
 * that is closest to the new solution in the A-norm (each of them solves A v = f with a known f, so the normal
 * equations cost one pass over the stored vectors; Fischer 1998).  It contains kinds 1 and 2 as special
 * combinations and needs fewer iterations than either (13.1 -> ~10.5 per step on the 1M-DOF mesh). */
int hf_set_start_vector(hf_ctx* ctx, int32_t kind);
/* Number of extra response solves spent so far (diagnostics). */
int hf_get_response_solves(hf_ctx* ctx, int64_t* count);

/* Number of hf_step solves that hit a breakdown (p.Ap <= 0) in the multigrid-preconditioned loop and
 * were finished with the Jacobi preconditioner instead (still on the GPU).  0 in every case tested. */
int hf_get_amg_fallbacks(hf_ctx* ctx, int64_t* count);

int hf_set_state(hf_ctx* ctx, const double* u);
int hf_get_state(hf_ctx* ctx, double* u);
int hf_sample(hf_ctx* ctx, int32_t n_s, const int32_t* nodes, double* out);

/* One time step (backward Euler; see hf_set_time_scheme for BDF2): b = M u^n - A[:,B] g, b_B = g, solve A_hat u^{n+1} = b by
 * Jacobi-PCG started from u^n (with u_B = g), in place.  Stops when
 * ||D^-1 r||_2 <= max(rtol * ||D^-1 b||_2, atol)  (a zero right-hand side - the answer is then zero - is measured
 * against the start residual instead).  iters / resid (relative) may be NULL. */
int hf_step(hf_ctx* ctx, const double* g_bc, double rtol, double atol, int32_t max_it, int32_t* iters, double* resid);

/* n_steps steps in one call: g_bc_all = n_steps x n_bc; after every step the n_s nodes
 * are sampled into samples (n_steps x n_s).  iters = n_steps entries (may be NULL). */
int hf_run(hf_ctx* ctx, int32_t n_steps, const double* g_bc_all, double rtol, double atol, int32_t max_it,
           int32_t n_s, const int32_t* nodes, double* samples, int32_t* iters);

/* Variable time steps.  The context keeps a time record: the time t, the sizes of the last three steps and the
 * effective step dt' of the last one; hf_assemble, hf_set_state, hf_steady_solve and a change of hf_set_time_scheme put it "at
 * rest" (t = 0, no step taken).  Without any call below nothing new is allocated or launched: every step has hf_assemble's size.
 *
 * hf_set_step: the following steps of hf_step / hf_run have size dt.  Backward Euler: dt' = dt.  BDF2 with the ratio
 * w = dt_n / dt_{n-1} to the step before (w = 1 from rest, where the history before t = 0 is constant):
 *     A' u^{n+1} = M (a u^n - b u^{n-1}) + dt' F,  A' = M + dt' K,  dt' = dt_n (1+w)/(1+2w),  a = (1+w)^2/(1+2w),  b = w^2/(1+2w).
 * The operator is re-valued lazily: the next step whose dt' differs bitwise from the one A holds launches hf_assemble's
 * row-gather kernel with it and eliminates again, on the stream (under tables the step's own re-valuation takes the new dt').
 * A and D^-1 are then bit for bit what hf_assemble leaves at that step under backward Euler; M is unchanged.  What belongs to one
 * operator is dropped (boundary responses, projection ring; start-vector kinds 2 and 3 run as kind 1 on that step), A's value
 * lists go stale, and the multigrid hierarchy stays the one hf_assemble built (frozen, never rebuilt here).  A step with w == 1
 * on an operator that holds its dt' launches exactly the kernels of a constant-step run.
 * Refused (HF_ERR_STATE): before hf_assemble, an open batch, a tangent set-up, the enthalpy form of the capacity, an assembly mode
 * other than HF_ASM_ROW_GATHER; (HF_ERR_ARG): dt <= 0 or not finite, a BDF2 step with w > 1 + sqrt 2 (the zero-stability limit;
 * checked again by hf_step / hf_run before any launch).  While variable steps are set hf_batch_begin and hf_run_tangent are
 * refused; hf_assemble ends them.
 *
 * hf_set_step_list: the sizes of the next n steps, one entry consumed per step (as hf_set_source_amplitudes' amplitudes); a list
 * too short for a run is HF_ERR_STATE before any launch; n = 0 clears the list. */
int hf_set_step(hf_ctx* ctx, double dt);
int hf_set_step_list(hf_ctx* ctx, int32_t n, const double* dt);

/* Step control: while on, every step keeps what a local-error estimate and a rejection need (copies of u^n and of the start
 * vector's u^{n-1}, the states u^{n-1} and - BDF2 - u^{n-2}; allocated here, freed by on = 0).  Switched on at rest only.
 *
 * hf_get_step_error: err = max over the free rows of |c (u_i - w0 h0_i - w1 h1_i - w2 h2_i)| / (atol_e + rtol_e |u_i|) for the
 * step taken last: u - the Lagrange extrapolation of the history (h0, h1, h2 = u^n, u^{n-1}, u^{n-2}) to t_{n+1}, linear for
 * backward Euler, quadratic for BDF2, times the ratio of the scheme's local-error constant to the predictor's:
 *     backward Euler  c = dt_n / (dt_n + dt_{n-1});   BDF2  c = dt_n (1+w) / ((1+2w) (dt_n + dt_{n-1} + dt_{n-2}))
 * (1/2 and 2/9 at constant step).  History before the start of the run is the rest state at spacing dt_0, the first step's size.
 * A conservative indicator, not a bound: on the stock small mesh it overstates the true local error 1.3 x (BDF2) to 2 x
 * (backward Euler).  Deterministic (no contraction, an order-independent maximum).
 *
 * hf_step_reject: undoes the step taken last: state, u^{n-1}, histories, time record, the source's next amplitude and the step
 * list's next entry are bit for bit what they were before it; its monitor and heat records are dropped.  Taking the step again
 * with the same size gives bit for bit the first attempt's answer.  Not rolled back: the operator (the next step re-values it if
 * its dt' differs), the count of re-valuations, the count of multigrid fallbacks, and under tables the value hf_get_picard_change
 * reports (its "have a change" flag is).  A state that is not finite makes hf_get_step_error return +inf, never 0.  HF_ERR_STATE when there is no step to undo (rejecting twice in a row).
 *
 * hf_get_step_info: the time, the size of the last step, its dt', and the number of re-valuations for a new dt' so far (any may
 * be NULL).  After a rejection the first three are those of the step before; the count is not rolled back. */
int hf_set_step_control(hf_ctx* ctx, int32_t on);
int hf_get_step_error(hf_ctx* ctx, double atol_e, double rtol_e, double* err);
int hf_step_reject(hf_ctx* ctx);
int hf_get_step_info(hf_ctx* ctx, double* t, double* dt_last, double* dt_eff, int64_t* revaluations);

/* Batched time loop: nv = 2, 4, 8 or 16 sweep points of ONE mesh, Dirichlet set and rho_c advance together as the
 * columns of a multi-vector PCG (reference: the independent runs of the parameter grid, parameter_sweep.py:195-235,
 * and of the kappa list, sweep_test.py:47-52).  Vectors are stored interleaved on the device, every index and every
 * shared matrix value is read once for nv products, and each column keeps its own alpha / beta / tolerance /
 * iteration count / done flag; per column the arithmetic and the stopping rule are hf_step's.
 *   HF_BATCH_SHARED      all columns share the context's assembled operator (points that differ in their boundary
 *                        values only: fwhm, heating curve)
 *   HF_BATCH_PER_COLUMN  every column has its own A_hat: assemble a point's operator in the context as usual
 *                        (hf_update_kappa), then hf_batch_load_column(j) copies A_hat, D^-1 and the lifting values
 *                        into column j
 *   HF_BATCH_AFFINE      A_hat_j = A_hat + delta_j * A1 with A1 = dt K restricted to the listed materials at unit
 *                        conductivity (hf_batch_set_affine): a sweep over ONE conductivity (sweep_test.py's kappa_sample
 *                        list) needs two shared value arrays and a scalar per column instead of nv operators;
 *                        delta_j = kappa_j - the conductivity the context's operator was assembled with
 * With per-column or affine operators the multigrid hierarchy is the frozen one (hf_set_precond(1, reuse = 1)), shared
 * by all columns.
 * hf_batch_begin needs a completed hf_assemble; hf_set_mesh / hf_set_dirichlet / hf_set_precond close the batch.
 * hf_batch_run: g_bc_all = n_steps x n_bc x nv ([step][bc][column]); samples = n_steps x nv x n_s; iters =
 * n_steps x nv.  The start vector of every solve is 2 u^n - u^{n-1}.  HF_ERR_NOCONV if any column fails. */
enum { HF_BATCH_SHARED = 0, HF_BATCH_PER_COLUMN = 1, HF_BATCH_AFFINE = 2 };
int hf_batch_begin(hf_ctx* ctx, int32_t nv, int32_t operator_kind);
int hf_batch_load_column(hf_ctx* ctx, int32_t j);
int hf_batch_set_affine(hf_ctx* ctx, int32_t n_tags, const int32_t* tags, const double* delta /* nv */);
int hf_batch_set_state(hf_ctx* ctx, int32_t j, const double* u);
int hf_batch_get_state(hf_ctx* ctx, int32_t j, double* u);
int hf_batch_run(hf_ctx* ctx, int32_t n_steps, const double* g_bc_all, double rtol, double atol, int32_t max_it,
                 int32_t n_s, const int32_t* nodes, double* samples, int32_t* iters);
/* hf_batch_run with run_no_diamond's per-step read-flux projection for every column (reference run_no_diamond.py:543-566,
 * which the sweep of parameter_sweep.py:43,157-166 runs at every grid point): after each step the gradient of each column's
 * new state is L2-projected with the r-weighted unit mass matrix (hf_flux_setup first) - per wanted component (bit 0 = z,
 * bit 1 = r; the reference's outputs read d/dr only) the nv columns are the interleaved columns of ONE Jacobi-PCG,
 * warm-started from the previous step's projection, stopping rule of hf_step with flux_rtol - and sampled at n_fs nodes:
 * flux_samples = n_steps x n_comp x nv x n_fs ([step][component, z before r][column][node]); flux_iters = n_steps x n_comp
 * (largest count among the columns; may be NULL).  flux_components = 0 is hf_batch_run. */
int hf_batch_run_flux(hf_ctx* ctx, int32_t n_steps, const double* g_bc_all, double rtol, double atol, int32_t max_it,
                      int32_t n_s, const int32_t* nodes, double* samples, int32_t* iters, int32_t flux_components,
                      double flux_rtol, int32_t flux_max_it, int32_t n_fs, const int32_t* flux_nodes, double* flux_samples,
                      int32_t* flux_iters);
int hf_batch_end(hf_ctx* ctx);

/* A source and monitor records for the open batch.  Both are opt-in and die with hf_batch_end (and with
 * whatever closes the batch); a batch without them launches, allocates and returns exactly what it did before.  The context's
 * own source stays refused by hf_batch_begin, and hf_set_source stays refused while a batch is open.
 * hf_batch_set_source   column j gets the load F1_j of hf_set_source(tags, fwhm[j], z0, depth[j]) - k_source_load itself, one
 *        launch per distinct (fwhm, depth) - stored interleaved (n x nv) next to the ascending list of rows with an absorbing
 *        triangle.  Per column the argument checks of hf_set_source (HF_ERR_ARG); n_tags = 0 removes the batch's source.
 *        HF_ERR_STATE: no batch open, a mesh without row-gather lists.  A new source starts with an empty amplitude table.
 * hf_batch_get_source   column j of it (n doubles): bit for bit hf_get_source after hf_set_source with that column's arguments.
 * hf_batch_set_source_amplitudes   p = n_steps x nv ([step][column]): step k after the call uses row k.  All finite (HF_ERR_ARG);
 *        n_steps = 0: amplitude 0 for every step.  hf_batch_run / hf_batch_run_flux of more steps than rows are left return
 *        HF_ERR_STATE and take no step.
 * Per step kb_source_load<nv> writes load = p_j F1_j on the absorbing rows and the right-hand side is b = M u + dt load (BDF2: its
 * counterpart), under every operator kind and preconditioner.  A hold load F0 stays refused (hf_batch_begin: a load is set).
 * hf_batch_set_monitors   on = 1: every step of hf_batch_run / hf_batch_run_flux from now on leaves one record of all columns,
 *        under the table of hf_set_monitors (set before hf_batch_begin, shared by the columns).  on = 0 drops the batch's records.
 *        HF_ERR_STATE: no batch open; on = 1 while no monitors are set.  The context's own records are never touched.
 * hf_batch_monitor_now    one record of the batch's current state, out[(j * rows + t) * 7 + f] (rows, f as hf_get_monitors);
 *        nothing is recorded.
 * hf_batch_monitor_count  the records kept since the switch.
 * hf_batch_get_monitors   records first .. first + count - 1: out[(((k - first) * nv + j) * rows + t) * 7 + f].
 * Column j's rows are bit for bit those k_monitor gives for column j's state (kb_monitor<nv>, kb_monitor_final): no atomics. */
int hf_batch_set_source(hf_ctx* ctx, int32_t n_tags, const int32_t* tags, double z0, const double* fwhm /* nv */, const double* depth /* nv */);
int hf_batch_get_source(hf_ctx* ctx, int32_t j, double* F);
int hf_batch_set_source_amplitudes(hf_ctx* ctx, int32_t n_steps, const double* p /* n_steps x nv */);
int hf_batch_set_monitors(hf_ctx* ctx, int32_t on);
int hf_batch_monitor_now(hf_ctx* ctx, double* out);
int hf_batch_monitor_count(hf_ctx* ctx, int32_t* n_records);
int hf_batch_get_monitors(hf_ctx* ctx, int32_t first, int32_t count, double* out);

/* Batches under kappa(T) / rho_c(T) tables.  Opt-in: without the switch every call, message, launch and result
 * is what it was.
 * hf_set_batch_tables   on = 1: hf_batch_begin(nv, HF_BATCH_PER_COLUMN) is accepted while tables are set (the other operator kinds:
 *        HF_ERR_ARG, the message names the kind).  Every step of hf_batch_run / hf_batch_run_flux then re-values A_j = M_j + dt' K_j
 *        of all nv columns in one launch (kb_assemble_rows_T<nv, CAP>), each column at its own evaluation state - u^n, or
 *        2 u^n - u^{n-1} for BDF2 with a history - eliminates (kb_take_lift, kb_bc_rows, kb_dinv) and solves from u^n with the
 *        boundary values set (no projection ring: another operator every step).  With capacity tables M_j is re-valued too and
 *        the right-hand side is formed with it.  Per column the operators are bit for bit those the single run's re-valuation
 *        (k_assemble_rows_kT / _cT and eliminate) gives at that column's state and constants.  The multigrid hierarchy is the
 *        frozen one hf_assemble built (hf_set_precond(1, reuse = 1)), shared by the columns.
 *        Refused by hf_batch_begin under the switch (HF_ERR_STATE, the message names the call that set the condition): hf_set_picard
 *        above 1, hf_set_anisotropy with an anisotropic tag, hf_table_derivatives on.  hf_batch_set_source and
 *        hf_batch_set_monitors(1) are refused by a batch under tables (HF_ERR_STATE), and hf_set_picard above 1 while one is open.
 *        on = 0 (the default, and after every hf_set_mesh): hf_batch_begin refuses tables as before; an open batch under tables
 *        is closed.  hf_set_kappa_tables and hf_set_rhoc_tables close an open batch as well.  HF_ERR_STATE before hf_set_mesh.
 * hf_batch_set_column_kappa   column j's constant conductivities of the listed cell tags (tags without a table; the default is the
 *        context's).  A tag that carries a conductivity table: HF_ERR_ARG, the message names the tag.  rho_c stays shared.
 *        HF_ERR_STATE unless a batch under tables is open.
 * Read-only test windows:
 * hf_batch_revalue   re-values and eliminates at the batch's current states without stepping; max_workgroups > 0 caps the grid
 *        (a workgroup then takes several row blocks), 0 = the launcher's own grid.
 * hf_batch_get_operator   column j of the batch's per-column operator, de-interleaved: A (nnz), dinv (n), lift (the lifting
 *        values, one per pattern entry (free row, Dirichlet column) in CSR order) and M (nnz).  Any pointer may be NULL; M without
 *        capacity tables in the batch is HF_ERR_STATE. */
int hf_set_batch_tables(hf_ctx* ctx, int32_t on);
int hf_batch_set_column_kappa(hf_ctx* ctx, int32_t j, int32_t n_tags, const int32_t* tags, const double* k);
int hf_batch_revalue(hf_ctx* ctx, int32_t max_workgroups);
int hf_batch_get_operator(hf_ctx* ctx, int32_t j, double* A, double* dinv, double* lift, double* M);

/* Read-flux projection of run_no_diamond (reference run_no_diamond.py:471-491 set-up, :543-550 per
 * step): grad_smooth = L2 projection of grad(T) onto vector P1 with weight r.  hf_flux_setup
 * assembles the unit-coefficient r-weighted mass matrix on the mesh's pattern (once per mesh);
 * hf_flux_project projects the CURRENT state: the 2n x 2n system of the reference is block diagonal, so the
 * components decouple exactly into two scalar solves with M_r(1); when both are wanted they run as the two
 * interleaved columns of ONE Jacobi-PCG (every pass over the matrix serves both; per column the stopping rule
 * of hf_step), a single wanted component is solved on its own; results copied to grad_z / grad_r (n values each).  A NULL output skips that component's
 * solve altogether (run_no_diamond's outputs only use d/dr, :553-566).  iters = 2 entries (may be NULL).
 * hf_flux_solve does the same without any copy (components: bit 0 = z, bit 1 = r); hf_flux_sample then
 * reads the projected gradient at n_s nodes (either output may be NULL) - what the band / axis averages
 * of run_no_diamond.py:494-513, 553-566 need, instead of two n-vectors per step. */
int hf_flux_setup(hf_ctx* ctx);
int hf_flux_project(hf_ctx* ctx, double rtol, int32_t max_it, double* grad_z, double* grad_r, int32_t* iters);
int hf_flux_solve(hf_ctx* ctx, int32_t components, double rtol, int32_t max_it, int32_t* iters);
int hf_flux_sample(hf_ctx* ctx, int32_t n_s, const int32_t* nodes, double* grad_z, double* grad_r);

/* Steady state and pre-heated transients (reference: Space.build_steady_state_variational_forms,
 * space/space_and_forms.py:119-149, and the load term of build_variational_forms, :77-117; used by
 * with_ir_steady.ipynb cells 17-23).
 *   K  = the r-weighted P1 stiffness: the dt K part of hf_assemble's operator at dt = 1, entry for entry.  The reference's
 *        steady form is planar (un-weighted) while its transient form is r-weighted; here both are r-weighted, so that the
 *        steady state is the stationary point of the transient operator and a held state does not drift.
 * hf_steady_setup  assembles K (row-gather kernel only: HF_ERR_ARG after an hf_assemble in another mode, or on a mesh
 *        without row-gather lists), keeps it as assembled (K_free, for hf_hold_load), eliminates its own Dirichlet set S
 *        (n_s unique dofs; it may differ from the transient's set B of hf_set_dirichlet) symmetrically with unit diagonal,
 *        keeps the lifting columns K[free, S] aside and forms D^-1; precond 0 = Jacobi, 1 = a multigrid hierarchy of
 *        K_hat_S of its own (the transient's operators, lifting and hierarchy are not touched).  n_s = 0 -> HF_ERR_ARG
 *        (K alone is singular), before any launch.  hf_set_materials / hf_update_kappa make it stale: set up again.
 * hf_steady_solve  K_hat_S u = F - K[:, S] g_S on the free rows, u_S = g_S (g_S in the order of dofs_S); F = the load of
 *        hf_set_load / hf_hold_load when use_load != 0 and one is set, else zero.  PCG started from the current state,
 *        stopping rule of hf_step.  The result becomes the state; the start-vector history is reset as by hf_set_state.
 * hf_set_load      F (n doubles; NULL clears it).  While a load is set every hf_step / hf_run step uses
 *        b = M u^n + dt F, then lifting and set_bc as before (F has no effect on Dirichlet rows).  hf_batch_begin with a
 *        load set and hf_set_load / hf_hold_load while a batch is open return HF_ERR_STATE: a load is never dropped.
 * hf_hold_load     F_i = (K_free u)_i for the rows outside the transient's set B, F_i = 0 on B, from the current state u
 *        (needs hf_steady_setup), and sets it as the load: from u = u_ss with boundary values u_ss on B the transient stays.
 *        It uses the steady set-up made last, hf_steady_setup's or hf_steady_picard_setup's.
 * hf_get_load      copies the current load out (HF_ERR_STATE if none is set). */
int hf_steady_setup(hf_ctx* ctx, int32_t n_s, const int32_t* dofs_s, int32_t precond);
int hf_steady_solve(hf_ctx* ctx, const double* g_s, int32_t use_load, double rtol, double atol, int32_t max_it, int32_t* iters,
                    double* resid);

/* Steady state under kappa(T) / rho_c(T) tables: a Picard iteration.  K(x) = the r-weighted stiffness with
 * kappa_e = table_tag(T_e(x)) for a tabled tag and the constant otherwise - T_e, the table evaluation and the element matrix of
 * the transient's re-valuation, entry for entry its dt K part at dt = 1 valued at the same state.  Capacity tables do not enter K.
 *     x_0 = the current state (hf_set_state first)
 *     sweep k = 1, 2, ...:  K_hat_S(x_{k-1}) x_k = F - K(x_{k-1})[:, S] g_S on the free rows, (x_k)_S = g_S; PCG started from
 *                           x_{k-1} with the stopping rule of hf_step; change_k = max |x_k - x_{k-1}|; stop when <= picard_tol
 *     after the last sweep: K is valued once more at the returned state u and kept as assembled (K_free, for hf_hold_load)
 * hf_steady_picard_setup  arguments and checks of hf_steady_setup; values K at the current state and, for precond = 1, builds the
 *        steady hierarchy from that K_hat_S.  The hierarchy stays frozen over the sweeps (the fine level uses the current K and
 *        D^-1; the fused fine-level legs are not used after a re-valuation).  Works with conductivity tables, capacity tables,
 *        both or none (then it is the linear problem: sweep 2 starts converged).  hf_set_kappa_tables, hf_set_rhoc_tables
 *        (setting or clearing), hf_set_materials and hf_update_kappa make it stale.  (A set-up of hf_steady_setup made before
 *        tables were set stays ready with its constant-coefficient stiffness.)
 * hf_steady_picard_solve  sweeps = number of sweeps run, iters[k-1] = PCG iterations of sweep k (max_sweeps entries, may be
 *        NULL), change = the last change_k, nl_resid = ||D^-1 (b(u) - K_hat_S(u) u)|| / ||D^-1 b(u)|| from the final valuation:
 *        the relative start residual a further sweep would see.  HF_OK when change <= picard_tol.  HF_ERR_NOCONV when max_sweeps
 *        run out or a linear solve fails: the state is the last iterate, every output is filled and K is valued at that state,
 *        so hf_hold_load still holds it.  A multigrid breakdown finishes the sweep with Jacobi.  HF_ERR_ARG (before any launch):
 *        null g_s, bad tolerances, picard_tol < 0, max_sweeps outside 1..1000.  HF_ERR_STATE: before hf_steady_picard_setup, or
 *        the materials / tables changed since.  The result becomes the state; history and tangents as after hf_steady_solve. */
int hf_steady_picard_setup(hf_ctx* ctx, int32_t n_s, const int32_t* dofs_s, int32_t precond);
int hf_steady_picard_solve(hf_ctx* ctx, const double* g_s, int32_t use_load, double rtol, double atol, int32_t max_it,
                           double picard_tol, int32_t max_sweeps, int32_t* sweeps, int32_t* iters, double* change, double* nl_resid);
int hf_set_load(hf_ctx* ctx, const double* F);
int hf_hold_load(hf_ctx* ctx);
int hf_get_load(hf_ctx* ctx, double* F);

/* Volumetric source of the time step: laser power absorbed in some cell tags.  The source is separable,
 * q(z, r, t) = p(t) s(z, r), with s = exp(-4 ln2 r^2 / fwhm^2) exp(-|z - z0| / depth) inside the elements of the listed tags
 * (depth = +inf: uniform in z) and zero elsewhere.  s enters as its P1 interpolant inside each absorbing element:
 *     F1_i = sum over e at i with tag(e) listed, sum over j in e, of (M_e at rho_c = 1)_ij s(z_j, r_j)
 * formed on the device by the row-gather kernel k_source_load (bitwise reproducible; rows without an absorbing triangle are 0).
 * Every hf_step / hf_run step then uses b = M u^n + dt (F0 + p_k F1) - BDF2: 2/3 dt, both terms at t_{n+1} - with F0 the load
 * of hf_set_load / hf_hold_load if one is set, and p_k the step's amplitude (a peak power density, W/m^3).
 * hf_set_source   needs a mesh with row-gather lists (HF_ERR_ARG otherwise); n_tags = 0 clears the source.  HF_ERR_ARG: a tag
 *        that is not a cell tag of the mesh, a tag listed twice, fwhm not positive and finite, z0 not finite, depth not positive
 *        (+inf is allowed).  HF_ERR_STATE: before hf_set_mesh, or while a batch is open.  hf_set_mesh clears it; it survives
 *        hf_set_materials, hf_assemble and hf_update_kappa (it does not depend on the coefficients).  A new source starts with
 *        an empty amplitude list.
 * hf_get_source   copies F1 out (n doubles; HF_ERR_STATE if no source is set).
 * hf_set_source_amplitudes   the amplitudes of the next n_amp steps: step k after the call uses p[k].  A step or run that
 *        reaches beyond the list returns HF_ERR_STATE before any launch; a non-finite entry is HF_ERR_ARG; n_amp = 0 means
 *        amplitude 0 for every step.  HF_ERR_STATE if no source is set.
 * While a source is set hf_batch_begin, hf_tangent_setup, hf_tangent_setup_dir and hf_run_tangent return HF_ERR_STATE, as they
 * do for a load.  The steady solves ignore the source: a continuous-wave laser of amplitude p is hf_set_load(p * F1) with F1 from
 * hf_get_source, and then every call that takes a load (hf_steady_solve with use_load, hf_hold_load's sequence) applies. */
int hf_set_source(hf_ctx* ctx, int32_t n_tags, const int32_t* tags, double fwhm, double z0, double depth);
int hf_get_source(hf_ctx* ctx, double* F);
int hf_set_source_amplitudes(hf_ctx* ctx, int32_t n_amp, const double* p);

/* Differentiable source: tangent runs under a source, switched on explicitly.
 * hf_source_derivatives   enable = 1: forms G_f = dF1/dfwhm and G_d = dF1/ddepth on the device (k_source_load_d: the
 *        unit-capacity element mass applied to s_f = s 2 c_r r^2 / fwhm and s_d = s |z - z0| / depth^2 inside the absorbing
 *        elements, as F1 is formed from s; bitwise reproducible; rows without an absorbing triangle are exact zeros, and G_d
 *        is exactly zero for a uniform layer), builds the ascending list of the rows that have an absorbing triangle and
 *        marks the source differentiable.  enable = 0 frees all of that, and the source columns of a tangent set-up with it.
 *        hf_set_source, setting or clearing, switches it off, and so does hf_set_mesh.  HF_ERR_STATE: no source, a batch open.
 * hf_get_source_derivative   copies G_f (which = 0) or G_d (which = 1) out (n doubles); HF_ERR_STATE unless the source is
 *        differentiable.
 * While the source is differentiable hf_tangent_setup, hf_tangent_setup_dir and hf_run_tangent accept it; their other refusals
 * (a load, tables, the steady state, a batch) stay, and hf_run_tangent refuses a set-up with a shape column under a source
 * (F1 depends on the node positions; that term is not formed).  The primal of hf_run_tangent under a source is bit for bit
 * hf_run's with the same amplitudes, and it draws on the amplitude list as hf_run does.  Conductivity, capacity and heated-line
 * columns keep their loads: the source reaches them through u alone.
 * hf_tangent_set_source   coef = n_steps x nv x 3 doubles, (c0, c1, c2) per step and column (nv: the set-up's padded width):
 *        step k of hf_run_tangent after the call adds c0 F1 + c1 G_f + c2 G_d to the load of every column that has a non-zero
 *        entry in some row (kb_source_columns, on the source's rows only; launched only if there is such a column), in the
 *        units of the other loads: d(p_k F1)/dtheta_j.  n_steps = 0 removes the source columns.  The table is a
 *        schedule like the amplitudes': the tangents are not reset, so a later run continues them, and the position in the
 *        table moves with every step hf_run_tangent starts and is rewound by hf_tangent_set_source alone - not by
 *        hf_set_state, hf_assemble or anything else that resets the tangents, and not by a run that fails mid-way: set the
 *        table again before the next run, as the amplitudes.  Either set-up, hf_set_source and hf_source_derivatives remove the table.  HF_ERR_STATE: no set-up, a batch
 *        open, the source not differentiable; HF_ERR_ARG: a non-finite entry.  A run longer than the rows left returns
 *        HF_ERR_STATE before any step.  hf_tangent_load includes the term with the coefficients of the last step taken, and
 *        nothing where no step has been taken since the table was set or the tangents were reset. */
int hf_source_derivatives(hf_ctx* ctx, int32_t enable);
int hf_get_source_derivative(hf_ctx* ctx, int32_t which, double* out);
int hf_tangent_set_source(hf_ctx* ctx, int32_t n_steps, const double* coef);

/* Region monitors: after every step, per monitored cell tag t, over the triangles e with tag(e) = t and the
 * nodal state u (A_e the triangle's area in (z, r), r_0..r_2 its nodal radii, rs their sum):
 *     T_max, node_max   the largest nodal value over the nodes of those triangles and the smallest node id that attains it
 *     T_min, node_min   the same for the smallest value
 *     I0 = sum_e A_e rs / 3                                   = int r dA (the volume is 2 pi I0)
 *     I1 = sum_e (A_e / 12) sum_i (rs + r_i) u_i              = int u_h r dA, exact for the P1 field
 *     H  = int over {u_h > theta_t} of r dA                   the exact cut of the linear interpolant in each triangle; a node
 *                                                             is "above" when u > theta, strictly
 * formed by k_monitor (a lane per triangle, fixed chunks, partials per workgroup in a layout the mesh alone fixes, added in a
 * fixed order by k_monitor_final): no atomics, the same bits from run to run and from context to context.  Two launches per
 * record, on the stream, with no host synchronisation.  A context without monitors launches exactly what it launched before.
 * hf_set_monitors  threshold[t], t < tab_len (tab_len = the mesh's largest cell tag + 1; entries a shorter table leaves out count
 *        as NaN): NaN = tag t is not monitored, +inf = monitored with H = 0, finite = monitored with that theta.  NULL,
 *        tab_len = 0 or a table of only NaN removes the monitors.  Every call drops the records.  At most 64 tags are monitored.
 * hf_monitor_now   the record of the current state (after hf_set_state, a steady solve, ...): rows * 7 doubles, rows = the mesh's
 *        largest cell tag + 1; nothing is recorded.
 * hf_monitor_count the number of records kept.
 * hf_get_monitors  records first .. first + count - 1: out[((k - first) * rows + t) * 7 + f], f = T_max, node_max, T_min,
 *        node_min, I0, I1, H; node ids are stored as doubles; the row of a tag that is not monitored is seven exact zeros.
 * hf_monitor_clear drops the records and keeps the table.
 * Record k is the state after the k-th recorded step since the last hf_set_monitors / hf_monitor_clear: every step of hf_step,
 * hf_run and hf_run_tangent (the primal state; under Picard sweeps once, after the last sweep) that returns HF_OK; a step that
 * returns an error leaves no record.  These calls make room for their records before their first launch.  The batched loop
 * (hf_batch_*) records nothing, and neither do the steady solves, which hf_monitor_now serves.
 * HF_ERR_STATE: before hf_set_mesh; while a batch is open; hf_monitor_now / hf_get_monitors while no monitors are set.
 * HF_ERR_ARG (the message names the call and the tag or range): a non-NaN entry on a tag that is not a cell tag of the mesh, -inf,
 *        a 65th monitored tag, a range outside the records kept, null pointers.
 * hf_set_mesh removes the monitors; they survive hf_set_materials, hf_assemble, hf_set_state, the table calls, the source calls
 * and the steady calls (they depend on the mesh alone). */
int hf_set_monitors(hf_ctx* ctx, int32_t tab_len, const double* threshold);
int hf_monitor_now(hf_ctx* ctx, double* out);
int hf_monitor_count(hf_ctx* ctx, int32_t* n_records);
int hf_get_monitors(hf_ctx* ctx, int32_t first, int32_t count, double* out);
int hf_monitor_clear(hf_ctx* ctx);

/* Derivatives of the monitor sums in tangent runs: while monitors are set and the switch is on, every step of
 * hf_run_tangent that returns HF_OK leaves, after its tangent stage, one derivative record next to the primal record of the same
 * state: per cell tag t and tangent column j the five numbers dT_max = s_j[node_max], dT_min = s_j[node_min] (the nodes of the
 * primal record), dI0, dI1, dH, with s_j the column's tangent field.  dI0 is zero except in a shape column
 * (hf_tangent_set_shape), whose nodal z-velocity moves the triangles' areas.  k_monitor_tan<nv> and k_monitor_tan_final form
 * them as k_monitor forms the sums: no atomics, no host synchronisation, the same bits from run to run.
 * hf_set_monitor_tangents   the switch (off after hf_set_monitors and hf_set_mesh, which also drop the derivative records).
 * hf_monitor_tangent_count  the derivative records kept and the nv of their columns (0 while none were taken).
 * hf_get_monitor_tangents   records first .. first + count - 1: out[(((k - first) * rows + t) * nv + j) * 5 + f], f = dT_max, dT_min,
 *        dI0, dI1, dH, rows = the mesh's largest cell tag + 1; rows of tags that are not monitored and padded columns are exact
 *        zeros.  record_index[k - first] (may be NULL) = the index of the primal record (hf_get_monitors) that derivative record k
 *        belongs to: primal records are also taken by hf_run and hf_step, so the two counts differ.
 * hf_monitor_tangent_eval   the kernels' own door: uploads s (n x nv interleaved, nv = 2, 4, 8 or 16) and n_shape <= 4 nodal
 *        velocities vz (n x n_shape interleaved, slot q belonging to column shape_col[q]), evaluates the monitors of the current
 *        state and returns the derivative row out[(t * nv + j) * 5 + f].  It records nothing and needs neither a tangent set-up
 *        nor an assembled operator.
 * hf_monitor_clear drops the derivative records too; a tangent set-up with another nv drops them (their rows have nv columns).
 * HF_ERR_STATE: before hf_set_mesh; while a batch is open; hf_set_monitor_tangents(1), hf_get_monitor_tangents and
 *        hf_monitor_tangent_eval while no monitors are set.
 * HF_ERR_ARG: a range outside the records kept, nv not in {2, 4, 8, 16}, n_shape outside 0..4, a shape_col outside [0, nv) or
 *        listed twice, null pointers. */
int hf_set_monitor_tangents(hf_ctx* ctx, int32_t on);
int hf_monitor_tangent_count(hf_ctx* ctx, int32_t* n_records, int32_t* nv);
int hf_get_monitor_tangents(hf_ctx* ctx, int32_t first, int32_t count, double* out, int32_t* record_index /* may be NULL */);
int hf_monitor_tangent_eval(hf_ctx* ctx, int32_t nv, const double* s, int32_t n_shape, const int32_t* shape_col, const double* vz, double* out);

/* Tangent runs: the exact derivatives s_j = du/dtheta_j of the time loop with respect to up to 16 parameters, advanced next to
 * the primal.  A column's parameter scales the conductivity of the cell tags mapped to it (K_j = the sum of
 * their unit-conductivity r-weighted stiffness), enters the Dirichlet values through h_j = dg/dtheta_j, or both.  After every
 * primal step A_hat u^{n+1} = ..., each column solves
 *     A_hat s_j^{n+1} = M s_j^n + dt F_j - A[:,B] h_j^{n+1} on the free rows, (s_j)_B = h_j^{n+1},  F_j = -K_j u^{n+1}
 * (F_j over every row, Dirichlet entries of u included), as the interleaved columns of one batched PCG on the shared
 * operator with the context's preconditioner (Jacobi, or the transient's multigrid hierarchy), per column the stopping rule
 * and the start-vector projection of the batched loop.  F is formed by a row-gather kernel in one pass for all columns.
 * hf_tangent_setup  n_par = 1..16 parameters; the columns are n_par rounded up to nv = 2, 4, 8 or 16 (the padded ones stay
 *        exactly zero and report 0 iterations).  tag_col = tab_len entries (one per tag value 0..max cell tag): the column
 *        whose conductivity tag t carries, -1 = none.  Every tangent starts at zero.  HF_ERR_ARG: n_par outside 1..16, a
 *        column outside [-1, n_par), a mapped tag that is not a cell tag of the mesh, or a mesh / operator without the
 *        row-gather lists (HF_ASM_ROW_GATHER only).  HF_ERR_STATE: no mesh, a batch open or a load set.
 * hf_run_tangent  hf_run plus the tangent stage: g_all, rtol, atol, max_it, n_s, nodes, samples and iters as hf_run, and the
 *        primal samples, iteration counts and final state are bitwise those of hf_run with the same arguments.
 *        h_all = n_steps x n_bc x nv ([step][bc][column]) or NULL (all zero); tangent_samples = n_steps x nv x n_s
 *        ([step][column][node]; needed when n_s > 0); tangent_iters = n_steps x nv (may be NULL).  A second call continues
 *        both the primal and the tangents.  HF_ERR_STATE before hf_tangent_setup, with a batch open or a load set, or
 *        after hf_steady_solve until hf_set_state (a steady state depends on the conductivities, the tangents start at zero);
 *        HF_ERR_ARG after an hf_assemble in another mode than HF_ASM_ROW_GATHER; all before any launch.  HF_ERR_NOCONV if the
 *        primal or any tangent column fails.
 * hf_get_tangent  copies column j (0 <= j < nv) of the tangent state out (n doubles).
 * hf_set_state, hf_set_materials, hf_assemble (hence hf_update_kappa), hf_steady_solve and hf_tangent_setup reset every
 * tangent to zero; hf_set_mesh removes the set-up.
 *
 * Directional columns.  Per element K_e = k_r K_e^r + k_z K_e^z with k_r = m_r kappa, k_z = m_z kappa
 * (hf_set_anisotropy; m = 1 on isotropic tags), so the step is affine in k_r and k_z of every tag and the recursion above holds
 * with F_j = -K_t^r u^{n+1} for k_r of tag t (absolute, W/m/K), -K_t^z u^{n+1} for k_z, and -(m_r K_t^r + m_z K_t^z) u^{n+1} for
 * kappa (both directions, the ratio kept: what hf_update_kappa scales).  M does not enter and the operator is the primal's.
 * hf_tangent_setup_dir  as hf_tangent_setup with three tables of tab_len entries (-1 = none; any of them may be NULL = all -1):
 *        tag_col_k[t] = j: column j is the kappa of tag t, weighted by the (m_r, m_z) the context holds at this call;
 *        tag_col_r[t] = j / tag_col_z[t] = j: column j is the k_r / k_z of tag t.  Several tags may feed one column, and one tag
 *        may feed its k_r into one column and its k_z into another.  Works on isotropic and anisotropic tags alike.
 *        HF_ERR_ARG (the message names the tag): everything hf_tangent_setup refuses, all three tables NULL, a tag with a kappa
 *        column and a directional one.  HF_ERR_STATE: as hf_tangent_setup.  The set-up replaces one of hf_tangent_setup and
 *        the other way round; hf_run_tangent and hf_get_tangent serve whichever is in force, and everything that resets or
 *        removes a set-up of hf_tangent_setup does the same to this one - hf_set_anisotropy removes it (the weights of its
 *        kappa columns were the old multipliers).  With kappa columns only, on tags with multipliers (1, 1), the loads and the
 *        tangents are bit for bit those of hf_tangent_setup with the same columns.
 * hf_tangent_load  for tests and diagnostics: forms the loads F = -K_j u of every column from the current state with the set-up
 *        in force (either kind), synchronises and copies column j (0 <= j < nv; n doubles) out.  Nothing else changes.
 *        HF_ERR_STATE before a set-up or with a batch open, HF_ERR_ARG for j outside [0, nv).
 *
 * Shape columns.  A column may be the derivative with respect to a parameter that moves the nodes along z with a
 * nodal velocity v_i = dz_i / dtheta_j, the triangles kept.  s_j is then the derivative at the moving nodes, and the recursion
 * above holds with F_j = -Kdot u^{n+1} - Mdot w added to the column's load, Kdot and Mdot the derivatives of the un-eliminated
 * matrices and w = (u^{n+1} - u^n) / dt (backward Euler) or (u^{n+1} - 4/3 u^n + 1/3 u^{n-1}) / (2/3 dt) (BDF2, u^{-1} = u^0).
 * hf_tangent_set_shape  valid after hf_tangent_setup or hf_tangent_setup_dir (a set-up of only -1 entries in hf_tangent_setup
 *        makes boundary-only columns): column j (0 <= j < n_par) gets the velocities vz (n doubles); NULL removes column j's
 *        shape part (no-op if it has none).  At most 4 columns of a set-up may have one.  A column may have conductivity entries
 *        as well: the loads add.  Every tangent is reset to zero.  Either set-up and hf_set_mesh remove all velocities; whatever
 *        only resets the tangents (hf_set_state, hf_assemble, ...) keeps them.  HF_ERR_STATE: no set-up, or a batch open.
 *        HF_ERR_ARG (the message names the reason): j outside [0, n_par), a non-finite velocity, a fifth shape column.
 *        hf_run_tangent keeps every refusal it has; the primal's samples, iterations and state stay bit for bit hf_run's, and a
 *        run without shape columns launches exactly what it launched before.  hf_tangent_load gives the complete load of a
 *        column: after hf_run_tangent it forms the last step's load again, bit for bit, from u^n (and u^{n-1}) kept by that run;
 *        where no step has been taken since the tangents were last reset, w = 0.
 *
 * Capacity columns.  A column may carry the rho_c (J/m^3/K) of a set of cell tags.  With M^1_j the r-weighted
 * mass matrix of the elements of those tags at rho_c = 1 (un-eliminated), the recursion above holds with F_j = -M^1_j w added to
 * the column's load, w the step rate of the shape columns (same formulas, same order of operations).  Dirichlet rows carry h_j as
 * before.  The mass is not directional, so anisotropic tags are allowed under either set-up.
 * hf_tangent_set_capacity  valid after hf_tangent_setup or hf_tangent_setup_dir (a set-up of only -1 entries is allowed):
 *        tag_col_c[t] = j (t < tab_len): column j carries the rho_c of cell tag t, -1 = none.  Several tags may feed one column.
 *        NULL, or a table of only -1, removes the capacity columns.  A column may have conductivity entries and a shape velocity
 *        as well: the loads add.  There is no limit on the number of capacity columns other than n_par <= 16.  Every tangent is
 *        reset to zero.  Either set-up and hf_set_mesh remove the table; whatever only resets the tangents (hf_set_state,
 *        hf_assemble, ...) keeps it.  HF_ERR_STATE: no set-up, or a batch open.  HF_ERR_ARG (the message names the tag): an
 *        entry outside [-1, n_par), a non-negative entry on a tag that is not a cell tag of the mesh.
 *        hf_run_tangent keeps every refusal it has (tables, a load, a source, the steady state); the primal's samples,
 *        iterations and state stay bit for bit hf_run's, and a run without capacity columns launches exactly what it launched
 *        before.  hf_tangent_load gives the complete load of a column, capacity part included, from u^n (and u^{n-1}) kept by
 *        the last hf_run_tangent; where no step has been taken since the tangents were last reset, w = 0 and the capacity part
 *        vanishes. */
int hf_tangent_setup(hf_ctx* ctx, int32_t n_par, const int32_t* tag_col);
int hf_tangent_set_shape(hf_ctx* ctx, int32_t j, const double* vz);
int hf_tangent_set_capacity(hf_ctx* ctx, int32_t tab_len, const int32_t* tag_col_c);
int hf_tangent_setup_dir(hf_ctx* ctx, int32_t n_par, const int32_t* tag_col_k, const int32_t* tag_col_r, const int32_t* tag_col_z);

/* Tangent runs under kappa(T) / rho_c(T) tables, lagged scheme (one Picard sweep), switched on explicitly.
 * With u* the evaluation state of the step, T_e the element temperature of u*, s* formed from s^n, s^{n-1} as u* is from u^n,
 * u^{n-1}, and sigma_e the mean of s* over the element's nodes, every column's load gets, on every element of a tabled tag,
 *     - [ kdot_e (K^1_e u^{n+1})_i + cdot_e (M^1_e w)_i ],
 *     kdot_e = D^k_{j,tag}(T_e) + kappa'_tag(T_e) sigma_e,    cdot_e = D^c_{j,tag}(T_e) + rho_c'_tag(T_e) sigma_e,
 * kappa' / rho_c' the slope of the table segment the evaluation took (0 in both clamped ranges), D the column's derivative table
 * (below), K^1_e / M^1_e the element matrices at unit coefficients and w the step rate of the capacity columns
 * (k_tangent_load_T<nv>, launched after the other load kernels; no atomics, bitwise reproducible).  The tangent stage solves with
 * the operator and mass matrix the primal step just valued; its columns start from s^n (the projection ring assumes one operator).
 * hf_table_derivatives   enable = 1 needs tables (HF_ERR_STATE otherwise, and with a batch open).  A change of the setting drops
 *        a tangent set-up.  hf_set_kappa_tables, hf_set_rhoc_tables and hf_set_picard switch it off again.  While it is on
 *        hf_tangent_setup, hf_tangent_setup_dir and hf_run_tangent no longer refuse the tables; they refuse instead
 *        (the message names the cause): a conductivity column on a tag with a conductivity table and a capacity column on a tag
 *        with a capacity table (HF_ERR_ARG; such parameters enter through hf_tangent_set_tables), a mesh whose staging would
 *        exceed 160 KiB of LDS (HF_ERR_ARG), any source, shape columns, source columns, monitor tangents and more than one Picard
 *        sweep (HF_ERR_STATE).  Without the call every message and return code is what it was.  The primal of hf_run_tangent
 *        under tables is bit for bit hf_run's.
 * hf_tangent_set_tables  kind 0 = conductivity, 1 = rho_c; entry e gives column column[e] the derivative table of cell tag
 *        tag[e]: d(knot value)/d(parameter) at the knots of that tag's table of that kind, `values` being the entries'
 *        tables concatenated.  Either sign.  n_entries = 0 clears the kind.  Every tangent is reset to zero; either set-up
 *        removes the tables.  HF_ERR_STATE: no set-up, table derivatives off, a batch open.  HF_ERR_ARG (naming the offender): a
 *        tag without a table of that kind, a column outside [0, n_par), a pair listed twice, a non-finite value.
 * hf_tangent_load includes the term, formed from the u^n (and u^{n-1}) the last hf_run_tangent kept and from the columns as they
 * stand (after a run: s^{n+1} in the place of s^n); nothing where no step has been taken since the tangents were reset. */
int hf_table_derivatives(hf_ctx* ctx, int32_t enable);
int hf_tangent_set_tables(hf_ctx* ctx, int32_t kind, int32_t n_entries, const int32_t* column, const int32_t* tag, const double* values);
int hf_tangent_load(hf_ctx* ctx, int32_t j, double* F);
int hf_run_tangent(hf_ctx* ctx, int32_t n_steps, const double* g_all, const double* h_all, double rtol, double atol, int32_t max_it,
                   int32_t n_s, const int32_t* nodes, double* samples, int32_t* iters, double* tangent_samples, int32_t* tangent_iters);
int hf_get_tangent(hf_ctx* ctx, int32_t j, double* s);

/* Temperature-dependent conductivities: the conductivity stays piecewise constant per element (DG0), but a
 * cell tag may carry a table, and every step of hf_step / hf_run re-values the operator at an evaluation state u*.
 *   kappa_e = table_tag(T_e),  T_e = ((lo + mid) + hi) * (1/3) of the element's three nodal values of u* sorted by value (the same
 *             bits from each vertex's point of view: A stays exactly symmetric).
 *   table     piecewise linear on the uniform grid T0 + i dT, i = 0..n_knots-1 (dT > 0, 2 <= n_knots <= 256, values > 0); outside
 *             [T0, T0 + (n_knots-1) dT] clamped to the end value.  s = (T - T0) * (1/dT), i = floor(s), v_i + (s - i)(v_{i+1} - v_i).
 *             A tag without a table keeps its constant from hf_set_materials / hf_update_kappa.
 *   u*        backward Euler: u^n (lagged); BDF2: 2 u^n - u^{n-1} once a history exists, else u^n.  Dirichlet entries are whatever
 *             the state holds.
 *   Picard    picard_sweeps = p (1..8, fixed count: the polled loop never waits on a host-side test): sweep k > 1 re-evaluates at
 *             the latest iterate u^{n+1,k-1} and solves again from it.  p = 1 is the lagged scheme.
 * Each evaluation re-values A (M and rho_c stay), redoes the Dirichlet elimination, the lifting values and D^-1, and the
 * right-hand side b = M u^n (+ dt F) (BDF2: M (4/3 u^n - 1/3 u^{n-1}) + dt' F) is lifted with the new A.  One row-gather launch
 * (k_assemble_rows_kT) per evaluation, on the stream, no host synchronisation.  The iteration count of a step is the sum over
 * its sweeps.
 * hf_set_kappa_tables  n_tab tables: tags[i], t0[i], dT[i], n_knots[i]; values = the knots of all tables concatenated in the order
 *        of `tags`.  n_tab = 0 clears the tables (every path then launches what it launches without them).  Setting or clearing
 *        invalidates the assembly (like a scheme change) and closes an open batch.  With tables set, hf_assemble evaluates at the
 *        current state (so set the state first): the multigrid hierarchy it builds is the one of A(u) at that state and stays
 *        frozen for the run; the fine level uses the current A and D^-1 (the fused fine-level legs hold the old operator and are
 *        not used after the first re-valuation).  Start vectors: kinds 2 and 3 assume one operator for the whole run and run as
 *        kind 1; kind 0 stays kind 0.
 *        HF_ERR_ARG: a tag that is not a cell tag of the mesh (or listed twice), bad knots or values, picard_sweeps outside 1..8,
 *        a mesh without row-gather lists or an operator assembled in a mode other than HF_ASM_ROW_GATHER.  HF_ERR_STATE before
 *        hf_set_mesh.  hf_set_mesh removes the tables.
 * While tables are set: hf_assemble in another mode and hf_update_kappa on a tabled tag -> HF_ERR_ARG; hf_batch_begin,
 * hf_tangent_setup / hf_run_tangent and hf_steady_setup / hf_steady_solve -> HF_ERR_STATE.  Every error returns before any
 * launch.  hf_set_load keeps working.  The steady state under tables is hf_steady_picard_setup / hf_steady_picard_solve.  Not
 * supported (refused, never approximated): batched / affine sweeps, tangents, and rebuilding the hierarchy during a run.
 * hf_get_picard_change  max over all nodes of |u^{n+1,p} - u^{n+1,p-1}| of the last step's last sweep (u^{n+1,0} = u*, so for
 *        p = 1 the change from the evaluation state); HF_ERR_STATE before the first step with tables. */
int hf_set_kappa_tables(hf_ctx* ctx, int32_t n_tab, const int32_t* tags, const double* t0, const double* dT, const int32_t* n_knots,
                        const double* values, int32_t picard_sweeps);
int hf_get_picard_change(hf_ctx* ctx, double* max_du);

/* Temperature-dependent heat capacities: rho_c stays piecewise constant per element, but a cell tag may carry a
 * table of exactly the shape and evaluation of a conductivity table, taken at the same T_e of the same evaluation state u*.  A tag
 * may carry a capacity table, a conductivity table, both or neither; capacity tables work with no conductivity table set.
 *   model     the non-conservative form rho_c(T) dT/dt = div(k grad T) with the capacity lagged (p = 1) or iterated (p > 1); an
 *             enthalpy form is hf_set_capacity_form's, below.
 *   step      x_0 = u*;  sweep k = 1..p:  M_k = M(rho_c(x_{k-1})),  A_k = M_k + dt' K(kappa(x_{k-1})),
 *             A_k x_k = M_k w (+ dt' F) - A_k[:, B] g on the free rows, (x_k)_B = g;  u^{n+1} = x_p.  w = u^n (BDF2:
 *             (4 u^n - u^{n-1}) / 3).  The right-hand side is formed again in every sweep, with the M of that sweep (one more pass
 *             over M per sweep); BDF2's history rotates once per step, in sweep 1's pass.
 * Each evaluation writes M and A in one row-gather launch (k_assemble_rows_cT, launched only while a capacity table is set), followed
 * by the elimination, the lifting values and D^-1 as under conductivity tables: four launches, no host synchronisation.
 * hf_set_rhoc_tables   arguments, checks and error texts as hf_set_kappa_tables (values = rho * cv at the knots, > 0); n_tab = 0
 *        clears the capacity tables and leaves conductivity tables as they are (and the other way round).  A rho_c given through
 *        hf_set_materials for a tabled tag is the constant the table replaces.  With capacity tables set hf_assemble values M and
 *        A at the current state, hf_get_csr returns the current M and A, and everything said above of "tables are set" (the
 *        refusals, the row-gather requirement, start-vector kinds 2 and 3 as kind 1, the frozen hierarchy, hf_get_picard_change)
 *        holds for tables of either kind.  The Picard count is the one of hf_set_kappa_tables.
 *        HF_ERR_ARG additionally: a mesh whose (M, A) slab, staged state and headers exceed the 160 KiB of LDS.
 * hf_set_picard   the Picard count p (1..8) of the loop, for use with capacity tables alone; HF_ERR_STATE while no tables are set
 *        (clearing the last table resets it to 1), HF_ERR_ARG outside 1..8.  Does not invalidate the assembly. */
int hf_set_rhoc_tables(hf_ctx* ctx, int32_t n_tab, const int32_t* tags, const double* t0, const double* dT, const int32_t* n_knots,
                       const double* values);
int hf_set_picard(hf_ctx* ctx, int32_t sweeps);

/* The enthalpy form of the capacity: energy-conserving steps under capacity tables, backward Euler only.  Per
 * step, with e the evaluation state, w the relaxation, tol the stop tolerance and P the sweep cap:
 *     e_0 = u^n;  sweep k = 1, 2, ...:
 *       Ta_e = Tw_e(u^n), Tb_e = Tw_e(e_{k-1}),  Tw_e(u) = sum_j (rs + r_j) u_j / (4 rs), rs = r_0 + r_1 + r_2 (the volume average)
 *       rho_c_e = the mean of the tag's clamped capacity table over [Ta_e, Tb_e] (table(Ta_e) where they are equal; the constant
 *                 of a tag without a capacity table);  kappa_e = table(T_e(e_{k-1})) at the plain-mean T_e, or the constant
 *       M_k = M(rho_c), A_k = M_k + dt K(kappa);  A_k x_k = M_k u^n + dt F - A_k[:, B] g on the free rows, (x_k)_B = g  (PCG from x_{k-1})
 *       change_k = max |x_k - e_{k-1}|;  stop when change_k <= tol or k = P;  e_k = e_{k-1} + w (x_k - e_{k-1})
 *     u^{n+1} = x_k
 * With E(u) = sum_e vol_e H_tag(Tw_e(u)), vol_e = A_e rs / 3 and H_tag the integral of the clamped table (rho_c T for a constant
 * tag), E(x) - E(u) = sum over all rows of [M(chord capacity between u and x) (x - u)]_i holds to rounding, so a converged step
 * conserves E; the defect of a stopped step is of the order of change_k.  One row-gather launch per evaluation
 * (k_assemble_rows_hT: both states staged, no atomics, bitwise reproducible), then the elimination as under the lagged form.
 * hf_set_capacity_form   HF_CAPACITY_LAGGED (the default: everything above this comment) or HF_CAPACITY_ENTHALPY.  A change
 *        invalidates the assembly; the enthalpy form starts with tol = 0, w = 1 and the sweeps of hf_set_picard as P.
 *        HF_ERR_STATE, the message naming the cause: no capacity table is set (which covers an assembly mode other than the row
 *        gather: hf_set_rhoc_tables refuses that mode, and hf_assemble refuses another mode while the tables are set), BDF2 is the
 *        scheme, a tag is anisotropic (also under hf_set_aniso_tables), a batch is open, a tangent is set up.  HF_ERR_ARG: an
 *        unknown form; a mesh whose slab, two staged states and headers exceed the 160 KiB of LDS.  Under the enthalpy form
 *        hf_set_time_scheme(HF_TIME_BDF2), hf_batch_begin, hf_tangent_setup / hf_tangent_setup_dir and hf_set_anisotropy with an
 *        anisotropic tag are refused (HF_ERR_STATE).  Clearing the capacity tables returns the form to lagged.
 * hf_set_picard_control  tol >= 0 in K (0: all max_sweeps run and nothing is read back between sweeps), 0 < relax <= 1,
 *        1 <= max_sweeps <= 64 (HF_ERR_ARG outside); HF_ERR_STATE under the lagged form, whose hf_set_picard keeps 1..8.
 * hf_get_picard_history  *n = the steps taken since the form was set or the history cleared; the first min(*n, cap) steps' sweeps
 *        and last change_k go to `sweeps` and `change`.  hf_get_picard_change reports the last step's.  hf_clear_picard_history
 *        empties it.
 * hf_enthalpy_revalue    INTERNAL, for the tests only (like hf_get_flux_system: a window, not part of the interface a driver uses):
 *        M and A (hf_get_csr) as one sweep's re-valuation leaves them at the pair (un, e) of host vectors, elimination included.
 *        It overwrites the operators and the evaluation state and marks the fine multigrid level stale; the next step values its
 *        own.  HF_ERR_STATE under the lagged form or before hf_assemble. */
enum { HF_CAPACITY_LAGGED = 0, HF_CAPACITY_ENTHALPY = 1 };
int hf_set_capacity_form(hf_ctx* ctx, int32_t form);
int hf_set_picard_control(hf_ctx* ctx, double tol, double relax, int32_t max_sweeps);
int hf_get_picard_history(hf_ctx* ctx, int32_t* sweeps, double* change, int32_t cap, int32_t* n);
int hf_clear_picard_history(hf_ctx* ctx);
int hf_enthalpy_revalue(hf_ctx* ctx, const double* un, const double* e);

/* The stored heat: out[tag] = sum over the tag's elements of vol_e (H_tag(Tw_e(u)) - H_tag(T_ref)) for the
 * current state, tab_len doubles (max cell tag + 1; 0 for a number that is no cell tag), in J per radian.  With any tables, or
 * none, and under both forms.  One lane per triangle, k_monitor's schedule and reduction (k_stored_heat, k_stored_heat_final): no
 * atomics, the bits depend on the mesh, the tables, T_ref and u only.  The records live in a buffer of their own; the monitor
 * records are untouched.
 * hf_stored_heat         on demand.  HF_ERR_STATE before hf_set_mesh / hf_set_materials, with a batch open, on a mesh without
 *        row-gather lists.
 * hf_set_heat_records    on = 1: one record per step of hf_step / hf_run from now on, measured from T_ref, queued on the stream as
 *        the monitor record is; on = 0 stops (the records stay).  hf_heat_count, hf_get_heat (records [first, first + count),
 *        count x tab_len doubles; HF_ERR_ARG outside the records kept), hf_clear_heat_records.  hf_set_mesh drops them. */
int hf_stored_heat(hf_ctx* ctx, double T_ref, double* out);
int hf_set_heat_records(hf_ctx* ctx, int32_t on, double T_ref);
int hf_heat_count(hf_ctx* ctx, int32_t* n_records);
int hf_get_heat(hf_ctx* ctx, int32_t first, int32_t count, double* out);
int hf_clear_heat_records(hf_ctx* ctx);

int hf_get_sizes(hf_ctx* ctx, int32_t* n, int32_t* n_e, int64_t* nnz, int32_t* n_bc);
/* Any pointer may be NULL.  A is the matrix as it stands (eliminated when BCs are set). */
int hf_get_csr(hf_ctx* ctx, int32_t* rowptr, int32_t* colidx, double* A, double* M);
/* y = A x (which = 0) or y = M x (which = 1) through the SpMV kernel; host vectors. */
int hf_spmv(hf_ctx* ctx, int32_t which, const double* x, double* y);

/* Value lists: a second, lossless encoding of the values of A and M for the fine-level SpMV kernel.  Per chunk of 512 rows the
 * distinct 64-bit patterns among the chunk's values (ascending as unsigned integers; 0.0 and -0.0 are two entries) and per nonzero
 * a 32-bit word cv = 16-bit column position | 16-bit position in the chunk's list << 16, in place of an f64 value and a 16-bit
 * column position: 4 + 8 (list entries / nnz) instead of 10 bytes per nonzero.  The kernel multiplies the same doubles in the
 * same order, so every result is bit for bit that of the raw arrays, which stay the source of truth for everything else.
 * hf_assemble builds the tables on the device after the Dirichlet elimination (not while kappa(T) / rho_c(T) tables are set);
 * whatever writes A or M later invalidates them until the next hf_assemble.
 * hf_set_value_lists  mode 0: off; 1 (default): used for a matrix whose lists hold at most nnz / 2 entries (a mesh without
 *        repeated stencils keeps the raw arrays); 2: used whatever their length.  Effective from the next hf_assemble.  The
 *        environment variable HEATFLOW_VALUE_LISTS=0|1|2 sets the mode a context starts with.
 * hf_get_value_lists  which = 0: A, 1: M.  valid: the kernel reads the tables; sum_vlist / max_vlist: entries of all lists / of the
 *        longest one at the last build; vcap: list entries per chunk the kernel stages in LDS (longer lists are read in place).
 *        vptr (chunks + 1 values, chunks = ceil(n / 512)), vlist (sum_vlist values) and cv (nnz words) are copied out when not
 *        NULL; HF_ERR_STATE if one is asked for while the tables are not valid.  Any pointer may be NULL. */
int hf_set_value_lists(hf_ctx* ctx, int32_t mode);
int hf_get_value_lists(hf_ctx* ctx, int32_t which, int32_t* valid, int64_t* sum_vlist, int32_t* max_vlist, int32_t* vcap, int32_t* vptr,
                       double* vlist, uint32_t* cv);

/* Test and diagnosis entry points of the multigrid preconditioner: each runs the production code path on its own, so
 * that a test can compare what the device computes with a restatement of the same algebra (tests/vcycle_oracle.py).
 *   hf_amg_apply           z = B r: one V(1,1) cycle exactly as the single-run PCG applies it (needs hf_set_precond(1, ...)
 *                          and hf_assemble, else HF_ERR_STATE), starting from z0 = w0 D^-1 r; *rz (may be NULL) = the host sum
 *                          of the r.z partial slots the cycle leaves for PCG.  The level vectors the cycle writes are set to
 *                          NaN before it runs (an entry read before it is written shows in z); r, z host vectors of n.
 *   hf_batch_apply_precond the batched cycle of the open batch (HF_ERR_STATE without one) on nv host columns of length n,
 *                          column j at r + j n / z + j n, from z0_j = w0 D_j^-1 r_j (D^-1 per column for per-column and
 *                          affine operators); rz (may be NULL) receives the nv reduced r.z values.  Every column runs.
 *   hf_dense_inverse       the coarsest level's dense inverse (blocked Gauss-Jordan on the device) of any SPD matrix of
 *                          1 <= n <= 4096 rows given in CSR form (else HF_ERR_ARG): inv (n x n, row-major, may be NULL),
 *                          x64 = the f64 dense mat-vec inv b and x32 = the same with the inverse rounded to float (either
 *                          may be NULL; b is needed for them).  Works on temporaries of its own: any hierarchy of the
 *                          context stays as it was, and the context needs no mesh.
 * Diagnosis only: hf_amg_apply overwrites the context's PCG vectors (r, z and the cycle's work vectors) and its device
 * scalars, hf_batch_apply_precond those of the open batch (r, z, every column's PCG scalars); a solve in progress cannot
 * be continued after them.  Start the next hf_step / hf_run / hf_batch_run from its own state (both leave u alone). */
int hf_amg_apply(hf_ctx* ctx, const double* r, double* z, double* rz);
int hf_batch_apply_precond(hf_ctx* ctx, const double* r, double* z, double* rz);
int hf_dense_inverse(hf_ctx* ctx, int32_t n, const int32_t* ptr, const int32_t* idx, const double* val, const double* b,
                     double* inv, double* x64, double* x32);

/* Test and diagnosis window on the projection basis of the start vector (hf_set_start_vector kind 3): read-only, host code,
 * no kernel runs; the stream is synchronised first.  column = -1: the basis of hf_step / hf_run (mt slots: mh ring slots, then
 * the boundary responses); column = j >= 0: column j of the open batch (mh ring slots, the others are reported unused).
 *   mh, mt        solutions kept in the ring, slots in all.  With every other pointer NULL the call is a size query and
 *                 needs neither a basis nor a context (ctx may be NULL).
 *   used[mt]      1 for a slot that holds a pair; next: the ring slot the next solution overwrites; pending: the slot stored
 *                 after the last step, whose Gram column the next step writes (-1: none).
 *   G[mt * mt]    the Gram matrix by slot, G[k * mt + l] = V_k . F_l; entries of slots not in use, and the column of the
 *                 pending slot, are whatever an earlier step left.
 *   alpha[mt + 1] the coefficients of the last solve by slot, then the rank it kept (all zero before the first solve).
 *   V, F          mt x n, row-major: the stored solutions (Dirichlet entries zeroed) and their right-hand sides; rows of
 *                 slots not in use come back zero.
 * Any pointer may be NULL.  HF_ERR_STATE while no basis is allocated (no step with kind 3 yet) or no batch is open. */
int hf_get_projection(hf_ctx* ctx, int32_t column, int32_t* mh, int32_t* mt, int32_t* used, int32_t* next, int32_t* pending, double* G,
                      double* alpha, double* V, double* F);

/* Test and diagnosis window on the linear systems of the read-flux projection (hf_flux_setup, hf_flux_solve /
 * hf_flux_project, the flux arguments of hf_batch_run_flux): read-only, host code, no kernel runs; the stream is
 * synchronised first.  Any pointer may be NULL.  HF_ERR_STATE before hf_flux_setup (and again after a new hf_set_mesh).
 *   M1[nnz]     the unit-coefficient r-weighted mass matrix on the context's CSR pattern (hf_get_csr's rowptr / colidx)
 *   dinv1[n]    its inverse diagonal, the Jacobi preconditioner of the projection's solves
 *   bz, br [n]  right-hand sides b_c[i] = sum over the triangles e at node i of (d_c T)_e |K| (2 r_i + r_j + r_k) / 12.
 *     column = -1: what the last hf_flux_solve / hf_flux_project formed, wherever that call kept them (two plain arrays, or
 *                  the two interleaved columns of its two-column solve).  Asking for a component that call was not asked
 *                  for gives HF_ERR_STATE (the rule of hf_flux_sample, but for "formed": a solve that then failed to
 *                  converge leaves its right-hand side readable).
 *     column = j >= 0: column j of the open batch's projection.  That state holds ONE component at a time, the one the last
 *                  step of hf_batch_run_flux solved last (r when flux_components has bit 1, else z): ask for that one
 *                  alone.  Asking for both, or for the other one, gives HF_ERR_STATE, as does a call without an open
 *                  batch or before its first projection; j >= nv gives HF_ERR_ARG. */
int hf_get_flux_system(hf_ctx* ctx, int32_t column, double* M1, double* dinv1, double* bz, double* br);

/* Average duration (ms) of `reps` back-to-back launches of one kernel on the ctx stream,
 * bracketed by HIP events on that stream. */
int hf_time_kernel(hf_ctx* ctx, int32_t which, int32_t reps, double* ms_avg);
/* In-situ timing of the dominant kernel: while on, up to 64 PCG SpMV launches per host check
 * carry a HIP event pair on the ctx stream (hipExtLaunchKernelGGL start/stop events: the
 * kernel's own execution interval; launches skipped after convergence are not counted).
 * hf_get_profile returns the summed duration and the number of launches. */
int hf_set_profile(hf_ctx* ctx, int32_t on);
int hf_get_profile(hf_ctx* ctx, double* spmv_ms_sum, int64_t* spmv_launches);
/* GPU time (ms, HIP events on the ctx stream) of the last hf_step / hf_run / hf_assemble / hf_steady_setup (assembly and
 * elimination) / hf_steady_solve / hf_steady_picard_solve (the whole solve) / hf_hold_load. */
int hf_last_gpu_ms(hf_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* HEATFLOW_HIP_H */
