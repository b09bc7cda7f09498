// hf_context.hpp - constants, the context struct and small host helpers of libheatflow_hip.so
// (HIP/CDNA4 gfx950 implementation of include/heatflow_hip.h).
//

#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "amg_host.hpp"
#include "heatflow_hip.h"

namespace {

constexpr int RB = 256;        // rows per chunk of the vector kernels
#ifndef HF_RBA
#define HF_RBA 256
#endif
constexpr int RBA = HF_RBA;    // CSR rows owned by one assembly workgroup (= its thread count); 512 measured 7 % slower
constexpr int TPB = 256;       // threads per workgroup = 4 wavefronts of 64
constexpr int NCOL = 32;       // max colours per row block (uint32 mask)
#ifndef HF_STAGE_U
#define HF_STAGE_U 2   // column-list entries per lane and pass while a chunk's operand slice is staged (k_spmv, C16)
#endif
#ifndef HF_UNROLL
#define HF_UNROLL 4
#endif
constexpr int MAXP = 1024;     // max workgroups per launch = partial-sum slots per array
constexpr int MAXRESP = 4;     // boundary-response directions kept per operator
// projection start vector (k_proj_* in hf_kernels.hpp): solutions kept in the ring, + boundary responses = vectors in all
#ifndef HF_PROJ_MH
#define HF_PROJ_MH 6
#endif
constexpr int PROJ_MH = HF_PROJ_MH;
constexpr int PROJ_MT = PROJ_MH + MAXRESP;
constexpr int TS = 512;        // SpMV workgroup: 512 threads = 8 wavefronts own 512 consecutive rows per chunk
// rows per chunk of the fine operator's LDS-staged SpMV (a workgroup of TS threads, one row per lane in the row phase;
// fewer rows than TS: more, shorter chunks per workgroup for the chunk pipeline) and its stream entries per lane in flight
#ifndef HF_SPMV_RPC
#define HF_SPMV_RPC 512
#endif
#ifndef HF_SPMV_UN
#define HF_SPMV_UN 8
#endif
constexpr int SRPC = HF_SPMV_RPC;
                               // (4 such workgroups per CU = 32 waves/CU; measured 20 % faster than 256x16)

// Host-visible progress of the running solve (pinned, mapped memory): written by the one thread that changes the
// device-resident scalars, so the host follows the convergence tests by reading its own memory - no copy, no
// synchronisation - and queues the next iteration while the current V-cycle is still running.
// `done` and `tested` carry the epoch of the solve that wrote them in their upper half (Scal::epoch, bumped by the host for
// every solve): launches of an earlier solve that are still queued when the host has moved on (the blind first burst can
// run past convergence) cannot be mistaken for progress of the current one, and the host never has to reset the mirror
// while something that writes it may still be in flight.
struct ScalMirror {
  double zz, bn2;
  int iters;                   // updates done when the last test ran
  int pad_;
  unsigned long long done_st;    // (epoch << 32) | Scal::done
  unsigned long long tested_st;  // (epoch << 32) | (iteration count whose iterate was tested last + 1); the start kernel writes + 1 = "0 tested"
};
inline int mirror_tested(const ScalMirror* m, unsigned epoch) {   // host side: -1 until the current solve's start kernel has run
  const unsigned long long v = __atomic_load_n(&m->tested_st, __ATOMIC_ACQUIRE);
  return static_cast<unsigned>(v >> 32) == epoch ? static_cast<int>(v & 0xffffffffu) - 1 : -1;
}
inline int mirror_done(const ScalMirror* m, unsigned epoch) {
  const unsigned long long v = __atomic_load_n(&m->done_st, __ATOMIC_ACQUIRE);
  return static_cast<unsigned>(v >> 32) == epoch ? static_cast<int>(v & 0xffffffffu) : 0;
}

struct Scal {                  // device-resident PCG scalars
  double tol2;                 // (max(rtol*||D^-1 b||, atol))^2
  double bn2;                  // ||D^-1 b||^2
  double zz;                   // ||D^-1 r||^2 of the last iterate
  int iters;
  int done;                    // 0 running, 1 converged, 2 breakdown
  int first;                   // 1 until the first update of a solve: the first direction is p = z (beta = 0)
  unsigned epoch;              // the host's count of solves on this context (k_pcg_begin / kb_begin): stamps what goes to the mirror
  ScalMirror* mirror;          // device address of the host mirror, or null (batched columns)
};

// Per-column scalars of the batched PCG (hf_batch.hpp), each reduced once per producer by a one-workgroup kernel
constexpr int NV_MAX = 16;    // columns of the widest batch
struct BRed { double pAp[NV_MAX], rz[2][NV_MAX], zz[NV_MAX], bn[NV_MAX]; };

// Conductivity table of one tag-dictionary entry (hf_set_kappa_tables): kappa(T) piecewise linear on the uniform grid
// t0 + i / inv_dt, i = 0..n-1, values vals[off + i], clamped to the end values outside it; n = 0: no table
constexpr int KT_MAX_KNOTS = 256;
constexpr int KT_MAX_PICARD = 8;
constexpr int KT_MAX_SWEEPS = 64;      // the sweep cap of the enthalpy form (hf_set_picard_control)
struct KTab { double t0, inv_dt; int n, off; };

// Directional tangent loads (hf_tangent_setup_dir): per tag-dictionary index the destination columns of the tag's radial and
// axial stiffness products (-1 = none) and their weights.  A column of k_r has (c, -1, 1, .), one of k_z (-1, c, ., 1), one of
// kappa (c, c, m_r, m_z): d/dkappa of k_r K^r + k_z K^z with k_r = m_r kappa, k_z = m_z kappa.
struct TanDir { int32_t c_r, c_z; double w_r, w_z; };

// The row-gather assembly kernels: k_assemble_rows<false / true>, k_assemble_rows_an<false / true>, k_assemble_rows_kT,
// k_assemble_rows_cT, k_assemble_rows_kT_K and the three table kernels on anisotropic tags (k_assemble_rows_kT_an, _cT_an, _kT_K_an).
// The policies name theirs from their template parameters: RowsConst<K, AN> RG_ROWS / RG_ROWS_K / RG_AN / RG_AN_K, RowsTable<CAP, K, AN>
// RG_KT / RG_CT / RG_KT_K and the *_AN three; RowsEnthalpy (k_assemble_rows_hT) RG_HT.
enum RgVariant { RG_ROWS, RG_ROWS_K, RG_AN, RG_AN_K, RG_KT, RG_CT, RG_KT_K, RG_SOURCE, RG_SOURCE_D, RG_SHAPE1, RG_SHAPE2, RG_SHAPE4, RG_TLT2, RG_TLT4, RG_TLT8, RG_TLT16, RG_KT_AN, RG_CT_AN, RG_KT_K_AN, RG_HT, RG_VARIANTS };

}  // namespace

struct hf_ctx {
  int dev = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::string err;
  double last_ms = 0.0;

  int32_t n = 0, ne = 0;
  int64_t nnz = 0;
  int nchunks = 0, P = 0;      // 256-row chunks and grid of the vector kernels / assembly
  int nchunks_s = 0, Ps = 0;   // 512-row chunks and grid of the SpMV kernel (Ps <= P partials)
  int max_chunk_nnz_s = 0;
  // compressed column indices of the fine operator (ColComp in hf_kernels.hpp): per SpMV chunk a sorted column list,
  // per nonzero a 16-bit position in it
  int32_t *d_cdict_ptr = nullptr, *d_cdict = nullptr;
  uint16_t* d_cid = nullptr;
  int max_cdict = 0;
  bool cdict_own = false;      // every chunk's own rows sit contiguously in its column list (each row stores its diagonal): the kernels take x[row] from the staged slice
  bool c16 = true;             // HEATFLOW_SPMV_C16=0 keeps the 32-bit column stream
  // value lists of sys.A ([0]) and d_M ([1]) (ValComp in hf_kernels.hpp): a second, lossless encoding of the same values for k_spmv
  // - per SpMV chunk the distinct 64-bit patterns of its values in ascending order, per nonzero the 16-bit position in that list
  // packed with the 16-bit column position.  Built at the end of hf_assemble (value_lists_build in hf_pattern.hpp); `src` is
  // the array the tables encode: launch_spmv takes them for that pointer only, and whoever writes the array afterwards clears
  // `valid` (value_lists_touch).
  struct ValueLists {
    const double* src = nullptr;
    int32_t *vptr = nullptr, *count = nullptr, *info = nullptr;   // list starts (nchunks_s + 1); list lengths; {sum, max} of the last build
    double* vlist = nullptr;
    uint32_t* cv = nullptr;        // cid | vid << 16 per nonzero
    int64_t cap = 0;               // entries `vlist` holds
    int64_t sum_vlist = 0;
    int max_vlist = 0;
    bool valid = false;
  } vl[2];
  int vl_mode = 1;             // HEATFLOW_VALUE_LISTS / hf_set_value_lists: 0 off, 1 on where the lists hold <= nnz / 2 entries, 2 always
  int vl_vcap = 0;             // list entries staged in LDS per chunk (longer lists are read from global memory)
  int vl_occ = 0;              // workgroups of the value-list kernel per CU at that footprint
  bool have_mesh = false, have_mat = false, assembled = false;
  double dt = 0.0;             // step of the assembled operator A = M + dt K: the step of hf_assemble (backward Euler) or 2/3 of it (BDF2)
  double dt_step = 0.0;        // the step hf_assemble was called with
  int mode = 0;
  int scheme = HF_TIME_BACKWARD_EULER;   // hf_set_time_scheme

  // host copies of the pattern (needed to build lifting structures and the multigrid hierarchy) and of the
  // elements (the lists of the LDS scatter kernels are built from them on first use)
  std::vector<int32_t> h_rowptr, h_colidx, h_tri, h_tag;
  std::vector<char> h_tag_used;
  bool owner_ready = false;

  // device: mesh
  double2* d_zr = nullptr;
  int4* d_elem = nullptr;
  int tab_len = 0;
  double *d_kappa = nullptr, *d_rhoc = nullptr;
  // device: pattern + owner lists
  int32_t *d_rowptr = nullptr, *d_colidx = nullptr;
  int32_t *d_blk_eptr = nullptr, *d_blk_cptr = nullptr;
  int2* d_blk_ent = nullptr;     // 3 x int2 per owner-list entry
  int nblk_a = 0;
  int max_blk_nnz = 0, ncolors = 0;
  int64_t elist_len = 0;
  // device: row-gather assembly lists (RowGather in hf_pattern.hpp) and coefficient tables by tag-dictionary index
  bool rg_ok = false;
  int4* d_rg_hdr = nullptr;
  uint16_t *d_rg_ell = nullptr, *d_rg_cid = nullptr;
  int32_t* d_rg_dict = nullptr;     // the blocks' column lists (global node ids)
  double2* d_rg_zrb = nullptr;      // coordinates of every block's column list (own rows + halo)
  int rg_max_dict = 0;
  int rg_grid[RG_VARIANTS] = {};    // persistent grid of each row-gather kernel on this mesh (0: not yet queried; launch_rowgather)
  int64_t n_rg_ell = 0, n_rg_dict = 0, n_cdict = 0;
  std::vector<int32_t> h_rg_tags;
  double *d_kappa_rg = nullptr, *d_rhoc_rg = nullptr;
  // Anisotropic conductivities (hf_set_anisotropy): multipliers (m_z, m_r) by tag-dictionary index for k_assemble_rows_an, which
  // runs in place of k_assemble_rows while `on` (some tag has m_z != 1 or m_r != 1); h_tag: that, by cell tag.
  struct Aniso {
    bool on = false;
    double2* d_m = nullptr;
    std::vector<char> h_tag;
    std::vector<double> h_m;    // (m_z, m_r) by cell tag, 1 where isotropic: the weights of a kappa column (hf_tangent_setup_dir)
    uint64_t hash = 0;          // of the multipliers by cell tag (0 while off): part of the operator's fingerprint (OperatorPrint)
  } an;
  bool batch_tables = false;   // hf_set_batch_tables: hf_batch_begin accepts tables (per-column operators, re-valued every step); hf_set_mesh resets it
  bool an_tables = false;     // hf_set_aniso_tables: tables and anisotropic tags together (the _an table kernels); hf_set_mesh resets it
  // device: the mass matrix (the operators that are solved with live in a System, below)
  double* d_M = nullptr;
  // device: vectors
  double *d_u = nullptr, *d_b = nullptr, *d_r = nullptr, *d_p = nullptr, *d_Ap = nullptr;
  double *d_uprev = nullptr, *d_ustart = nullptr;   // u^{n-1} and the buffer of the next start vector (rotated with d_u)
  bool have_prev = false;
  bool bdf_hist = false;       // BDF2: d_uprev holds u^{n-1} of the current trajectory (false: a rest start, u^{n-1} = u^n)
  int extrapolate = 1;         // start PCG from 2 u^n - u^{n-1} (same answer, fewer iterations)
  // hf_set_start_vector kind 2: boundary-response correction of the start vector.  Host copies of the last two
  // boundary vectors, an orthonormal set of directions seen in their second difference and, per direction d,
  // the device vector w = R d (A_hat w = -lift(d), w_B = d).
  int start_kind = 3;
  std::vector<double> h_g0, h_g1;   // g^n, g^{n-1}
  int g_hist = 0;
  struct BcResponse { std::vector<double> dir; double* w = nullptr; };
  std::vector<BcResponse> resp;
  long long resp_solves = 0;
  // hf_set_start_vector kind 3: Galerkin projection on the last solutions and the boundary responses (k_proj_*)
  struct Proj {
    double *V[PROJ_MT] = {nullptr}, *F[PROJ_MT] = {nullptr};   // slots 0..PROJ_MH-1: ring of (solution with zeroed Dirichlet entries, its right-hand side); then the responses
    bool used[PROJ_MT] = {false};
    int next = 0, pending = -1;   // ring slot to overwrite next; slot whose Gram column is still to be computed
    double *G = nullptr, *alpha = nullptr, *part = nullptr;
    bool ready = false;
  } proj;
  double *d_tmp = nullptr;
  // device: reductions
  double *d_part_pAp = nullptr, *d_part_rz = nullptr, *d_part_zz = nullptr, *d_part_bn = nullptr;
  Scal* d_scal = nullptr;
  Scal* h_scal = nullptr;      // pinned
  ScalMirror* h_mirror = nullptr;   // pinned + mapped; d_mirror is its device address
  ScalMirror* d_mirror = nullptr;
  unsigned epoch = 0;          // solves started on this context (Scal::epoch)
  int32_t* d_samp_idx = nullptr;
  double* d_samp = nullptr;
  int samp_cap = 0;
  // multigrid preconditioner (hf_set_precond): device hierarchy
  int amg_reuse = 0;           // 1: keep the coarse levels across hf_assemble calls (kappa sweeps)
  struct DevCsr {
    int nrow = 0, ncol = 0, lanes = 8; int64_t nnz = 0; int32_t *ptr = nullptr, *idx = nullptr; double* val = nullptr;
    float* valf = nullptr;                     // single-precision values (transfer operators of the preconditioner); val is then null
    int max_row = 0;
    int rpc = 0, nchunks = 0, chunk_nnz = 0;   // LDS-staged (stream) kernel geometry; rpc = 0 -> use the sub-wave kernel
    int32_t *dptr = nullptr, *dict = nullptr;  // stream kernel with compressed columns: per-chunk column lists ...
    uint16_t* cid = nullptr;                   // ... and a 16-bit position per nonzero
    int max_dict = 0;
    int64_t ndict = 0;                         // entries of `dict` (all chunks)
  };
  // Levels 1..nl-2 run the cycle through the fused legs Rt / GP (amg_host.hpp): `cat` = [b_l ; result of level l+1]
  // is GP's operand, `b` aliases its head; a level's result goes to `res` (the tail of the finer level's cat,
  // or the level's own x on level 1).  The coarsest level owns a zero-padded b (the dense solve reads pairs).
  struct DevLevel {
    DevCsr A, P, R, Rt, GP;
    double *dinv = nullptr, *x = nullptr, *cat = nullptr, *b = nullptr, *res = nullptr;
    bool own_b = false;
    double omega = 0; int n = 0;
  };
  int amg_fuse0 = 0;                 // finest level of the V-cycle: 0 explicit sweeps, 1 fused legs Rt_0 / GP_0, 2 fused down leg only (chosen by size in build_amg; HEATFLOW_AMG_FUSE0 overrides)
  bool amg_f32 = true;               // operators of the preconditioner below the fine level stored in float (HEATFLOW_AMG_F32=0: double)
  // what the fine operator the hierarchy was built from depends on besides the mesh (hf_amg_io.hpp): time step, coefficient
  // tables, Dirichlet set - compared with the context's own operator whenever a kept or installed hierarchy meets a new hf_assemble
  struct OperatorPrint { double dt = 0.0; std::vector<double> kappa, rhoc; int32_t nbc = 0; uint64_t bc_hash = 0; int32_t scheme = 0; uint64_t an_hash = 0; };
  long long amg_fallbacks = 0;   // steps finished by Jacobi-PCG after a multigrid-PCG breakdown
  // An eliminated operator on the mesh's pattern and what solves it: its Dirichlet set with the lifting columns A[free, set],
  // D^-1, the choice of preconditioner and a multigrid hierarchy of its own.  The context holds two, the transient's
  // A = M + dt K (`sys`) and the steady K_hat_S (`steady.sys`); the lifting, elimination, multigrid set-up and PCG code takes
  // the one it works on as an argument.
  struct System {
    int32_t nbc = 0;
    int32_t* bc_dofs = nullptr;
    double* g = nullptr;         // boundary values of the current solve
    int32_t nlift_rows = 0, nlift = 0;
    int32_t *lift_rows = nullptr, *lift_ptr = nullptr, *lift_bc = nullptr, *lift_slot = nullptr;
    double* lift_val = nullptr;
    double *A = nullptr, *dinv = nullptr;
    int precond = 0;             // 0 Jacobi, 1 smoothed-aggregation AMG V(1,1)
    int pred_iters = 0;
    std::vector<DevLevel> amg;
    double* coarse_inv = nullptr;
    float* coarse_inv_f = nullptr;     // the same in single precision (amg_f32)
    int coarse_n = 0, coarse_ld = 0;   // dense inverse, row-major, leading dimension a multiple of 4 (16-byte row loads)
    bool amg_ready = false;
    bool amg_fine_stale = false;       // frozen hierarchy (reuse) and the fine operator re-valued since it was built: the fused down leg Rt_0 no longer matches A
    double amg_opc = 0.0, amg_setup_s = 0.0;
    OperatorPrint amg_print;
  } sys;
  // steady state (hf_steady_setup / hf_steady_solve): the stiffness K on the pattern as assembled (Kfree, for hf_hold_load) and,
  // with its own Dirichlet set S eliminated, as a System of its own (sys), which the solver code is given in place of the
  // transient's.
  // picard: the set-up made last is hf_steady_picard_setup's - K and Kfree are valued at a state through the tables
  // (k_assemble_rows_kT_K) and go stale with the tables as well as with the materials.
  struct Steady {
    bool ready = false;
    bool picard = false;
    KTab* hdr0 = nullptr;                   // 64 empty table headers, for a Picard set-up while no table is set
    double* xprev = nullptr;                // the iterate a Picard sweep started from (for the change)
    unsigned long long* change = nullptr;   // max |x_k - x_{k-1}| of the last sweep (bits of a double >= 0)
    double* Kfree = nullptr;
    System sys;
  } steady;
  // load term of the time step (hf_set_load / hf_hold_load): b = M u^n + dt F
  double* d_load = nullptr;
  bool have_load = false;
  // volumetric source of the time step (hf_set_source): b = M u^n + dt (F0 + p_k F1), F0 the load above (if any), F1 = the
  // source's load at unit amplitude (k_source_load) and p_k the amplitude of the k-th step after hf_set_source_amplitudes
  struct Source {
    bool on = false;
    double* F1 = nullptr;        // n doubles
    double* sum = nullptr;       // F0 + p_k F1 of the current step (allocated by the first step that has a load too)
    int32_t* absorb = nullptr;   // 64 flags by row-gather tag-dictionary index
    std::vector<double> amp;     // amplitudes of the next steps; empty: amplitude 0
    size_t next = 0;             // the next step's index into amp
    double fwhm = 0.0, z0 = 0.0, depth = 0.0;   // as given to hf_set_source
    // differentiable source (hf_source_derivatives).  Nothing below is allocated while `diff` is false.
    bool diff = false;
    double *Gf = nullptr, *Gd = nullptr;   // dF1/dfwhm, dF1/ddepth (k_source_load_d), n doubles each
    int32_t* rows = nullptr;     // the rows with an absorbing triangle, ascending
    int nrows = 0;
  } src;
  // region monitors (hf_set_monitors, hf_monitor.hpp): per monitored cell tag a record row after every step of hf_step / hf_run /
  // hf_run_tangent.  Nothing below is allocated, and nothing is launched, while no monitors are set.
  struct Monitor {
    bool on = false;
    int nd = 0;                  // monitored tags = entries of the monitor dictionary (ascending cell tag)
    int nchunks = 0, grid = 0;   // chunks of MON_T triangles; workgroups of k_monitor = partials per dictionary index (from the mesh alone)
    uint8_t* slot = nullptr;     // tab_len entries: dictionary index of a cell tag, 255 = not monitored
    int32_t* tags = nullptr;     // 64 entries: the cell tag of a dictionary index
    double* theta = nullptr;     // 64 thresholds by dictionary index (+inf: H = 0)
    double* part_f = nullptr;    // 5 x grid x 64 doubles: I0, I1, H, the largest and the smallest value of every workgroup
    int32_t* part_i = nullptr;   // 2 x grid x 64: their nodes
    double* rec = nullptr;       // cap records of tab_len x 7 doubles
    double* now = nullptr;       // one record, for hf_monitor_now
    int64_t cap = 0, count = 0;
    // derivative records (hf_set_monitor_tangents): per record rows x tnv x 5 doubles, taken by hf_run_tangent after
    // the tangent stage of every step.  Nothing below is allocated, and nothing is launched, while the switch is off (the partials
    // also serve hf_monitor_tangent_eval, which allocates them on its first call).
    bool tan_on = false;
    int tnv = 0;                 // columns of a derivative record: the nv of the tangent set-up the records were taken under
    double* tpart = nullptr;     // nd x (2 x 16 + 4) x grid doubles: dI1, dH per column and dI0 per shape slot of every workgroup
    double* trec = nullptr;      // tcap records of tab_len x tnv x 5 doubles
    int64_t tcap = 0, tcount = 0;
    std::vector<int32_t> tindex; // the primal record each derivative record belongs to
  } mon;
  double *d_z = nullptr, *d_z2 = nullptr;
  // read-flux projection (hf_flux_setup): unit-rho_c r-weighted mass matrix and the projected gradient
  bool flux_ready = false;
  int flux_valid = 0;          // components (bit 0 z, bit 1 r) the last projection solved
  int flux_formed = 0;         // components whose right-hand side the last hf_flux_solve formed (hf_get_flux_system)
  bool flux_formed_pair = false;   // ... as the two interleaved columns of fluxb.b (else d_bz / d_br)
  int fluxnb_comp = -1;        // component whose right-hand sides fluxnb.b holds (0 z, 1 r; -1: no batched projection yet)
  double *d_M1 = nullptr, *d_dinv1 = nullptr, *d_gz = nullptr, *d_gr = nullptr, *d_bz = nullptr, *d_br = nullptr;
  int pred_flux[2] = {0, 0};
  // batched time loop (hf_batch_*, hf_batch.hpp): NV sweep points as interleaved columns
  struct BatchLevel { double *x = nullptr, *cat = nullptr, *b = nullptr, *res = nullptr; bool own_b = false; };
  struct Batch {
    int nv = 0;                  // 0: no batch open
    int opk = 0;                 // fine operator of the columns: 0 shared (ctx->sys.A), 1 one per column, 2 affine A + d_j A1
    const double *sysA = nullptr, *sysDinv = nullptr;   // shared operator other than ctx->sys.A (the flux projection's mass matrix)
    double *A = nullptr, *dinv = nullptr, *lift_val = nullptr;            // per-column operator data (opk 1; dinv also opk 2)
    double *A1 = nullptr, *lift1 = nullptr;                               // affine part and its lifting values (opk 2)
    double delta[NV_MAX] = {};
    double *g = nullptr;                                                   // boundary values of all steps
    double *u = nullptr, *uprev = nullptr, *ustart = nullptr, *b = nullptr, *r = nullptr, *p = nullptr, *Ap = nullptr;
    double *z = nullptr, *z2 = nullptr, *tmp = nullptr;
    double *part_pAp = nullptr, *part_rz = nullptr, *part_zz = nullptr, *part_bn = nullptr;
    Scal *scal = nullptr, *h_scal = nullptr;
    ScalMirror *h_mirror = nullptr, *d_mirror = nullptr;   // per-column progress for the host (pinned + mapped), hf_batch_begin only
    unsigned epoch = 0;          // solves started on this batch state (Scal::epoch of every column)
    BRed* red = nullptr;         // per-column reduced scalars
    std::vector<BatchLevel> lev;
    int Pb = 0, pred_iters = 0;
    bool have_prev = false;
    bool bdf_hist = false;       // BDF2: uprev holds every column's u^{n-1} (false: u^{n-1} = u^n)
    // projection start vector per column: ring of (solutions with zeroed Dirichlet entries, right-hand sides)
    double *pV[PROJ_MH] = {nullptr}, *pF[PROJ_MH] = {nullptr}, *pG = nullptr, *palpha = nullptr, *ppart = nullptr;
    bool pused[PROJ_MH] = {false};
    int pnext = 0, ppending = -1;
    unsigned loaded = 0;         // bit j: column j's operator has been loaded (percol)
    bool lds = false;            // fine-pattern products through kb_spmv_lds (the context's `bcols` tables are for this nv)
    const double* load = nullptr;   // per-column load F (interleaved): b = M u + dt F (the tangent stage); null: b = M u
    bool noproj = false;         // the operator changes from step to step (tangent runs under tables): the ring is neither combined from nor stored into
    // a batch under tables (hf_set_batch_tables): every step re-values A (and, with capacity tables, M) of every
    // column at the column's own state (kb_assemble_rows_T).  Nothing below is allocated while `tables` is false.
    bool tables = false;
    double* M = nullptr;         // per-column mass matrices, interleaved like A (capacity tables only; else M stays the shared d_M)
    double* kcol = nullptr;      // [64][nv]: column j's constant conductivity by tag-dictionary index (hf_batch_set_column_kappa)
    std::vector<double> h_kcol;  // its host copy
    int rv_grid = 0;             // persistent grid of kb_assemble_rows_T for this batch (0: not yet queried)
  } batch;
  // compressed columns of the batched loop's LDS-staged SpMV (BComp in hf_batch.hpp): per chunk of `rpc` rows a sorted
  // column list and per nonzero a 16-bit position in it; built on the first hf_batch_begin with a given nv, kept per mesh
  struct BatchCols {
    int nv = 0, rpc = 0, nchunks = 0, cap_nnz = 0, cap_dict = 0;
    int32_t *ptr = nullptr, *dict = nullptr, *own = nullptr;
    uint16_t* id = nullptr;
  } bcols;
  // source of the open batch (hf_batch_set_source): per column the load at unit amplitude and a table of
  // amplitudes; kb_source_load<nv> forms `load` = p_j F1_j on the absorbing rows before every step's right-hand side, and
  // batch.load points at it while the source is on.  Nothing below is allocated, and nothing is launched, while it is off; it
  // dies with the batch (free_batch).
  struct BatchSource {
    bool on = false;
    double* F1 = nullptr;        // n x nv, interleaved
    double* load = nullptr;      // n x nv, interleaved: zeroed once, only the absorbing rows are ever written
    int32_t* rows = nullptr;     // the rows with an absorbing triangle, ascending
    int nrows = 0;
    double* amp = nullptr;       // steps x nv amplitudes of the next steps, on the device; steps = 0: amplitude 0
    int64_t steps = 0, next = 0;
  } bsrc;
  // monitor records of the open batch (hf_batch_set_monitors): the context's table (mon.slot, mon.tags, mon.theta
  // and the schedule mon.nchunks / mon.grid), partials and records of its own.  Nothing below is allocated, and nothing is
  // launched, while the switch is off; it dies with the batch.
  struct BatchMonitor {
    bool on = false;
    double* part_f = nullptr;    // nd x grid (I0), then 4 x nd x nv x grid doubles: I1, H, the largest and the smallest value
    int32_t* part_i = nullptr;   // 2 x nd x nv x grid: their nodes
    double* rec = nullptr;       // cap records of nv x tab_len x 7 doubles
    double* now = nullptr;       // one record, for hf_batch_monitor_now
    int64_t cap = 0, count = 0;
  } bmon;
  Batch fluxb;                   // two-column state of the read-flux projection (both components in one PCG)
  Batch fluxnb;                  // nv-column state of the batched loop's read-flux projection (hf_batch_run_flux): one gradient component of every column per PCG
  int32_t* d_fsamp_idx = nullptr;   // its sample nodes
  // tangent runs (hf_tangent_setup / hf_run_tangent): nv tangent columns s_j = du/dtheta_j in their own batch state, which
  // the tangent stage of every step hands to the batched loop; their load F_j = -K_j u^{n+1} (k_tangent_load, or
  // k_tangent_load_dir under hf_tangent_setup_dir)
  Batch tanb;
  struct Tangent {
    bool ready = false;
    int npar = 0, nv = 0;
    int32_t* col = nullptr;      // tangent column of each row-gather tag-dictionary entry (64), -1 = none
    TanDir* dir = nullptr;       // hf_tangent_setup_dir: columns and weights per direction instead (64; k_tangent_load_dir), col stays null
    double* F = nullptr;         // n x nv, interleaved
    bool steady_state = false;   // the state comes from hf_steady_solve (it depends on kappa; s^0 = 0 would be wrong) until hf_set_state
    std::vector<int64_t> lev_sig;   // multigrid level sizes tanb.lev was laid out for
    // shape columns (hf_tangent_set_shape): up to 4 columns carry a nodal z-velocity; k_tangent_load_shape<ns>
    // adds their part of the load.  Nothing below is allocated or touched while no column has one (ncol == 0).
    struct Shape {
      int ncol = 0, ns = 0;            // columns with a velocity; slots of the kernel (1, 2, 4)
      int32_t col[4] = {0, 0, 0, 0};   // F column of each slot (a slot past ncol repeats slot 0's with zero velocities)
      std::vector<double> h_v[4];      // the velocities of slot s, as given
      double* d_v = nullptr;           // n x ns, interleaved by node
    } sh;
    // capacity columns (hf_tangent_set_capacity): a column carries the rho_c of a set of cell tags;
    // k_tangent_load_cap<nv> subtracts M^1_j w from the columns of `cmask`.  Nothing is allocated or launched while cmask == 0.
    int32_t* ccol = nullptr;         // capacity column of each row-gather tag-dictionary entry (64), -1 = none
    unsigned cmask = 0;              // bit j: some tag gives its rho_c to column j
    // the step rate w = (u^{n+1} - u^n) / dt (BDF2: its three-level form) of the shape and the capacity columns' loads: allocated,
    // and copied by every step of hf_run_tangent, exactly while a column of either kind is set (tangent_rate_buffers)
    double *un = nullptr, *um1 = nullptr;   // u^n and u^{n-1} of the last step of hf_run_tangent (copies, kept for the load)
    int wmode = 0;                   // of that step: 0 = none taken since the last reset, 1 = backward Euler, 2 = BDF2
    bool hist = false;               // um1 holds u^{n-1} (false: a rest start, u^{n-1} = u^n)
    // source columns (hf_tangent_set_source): per step and column (c0, c1, c2); kb_source_columns<nv> adds
    // c0 F1 + c1 G_f + c2 G_d to the columns of `smask` on the source's rows.  Nothing is allocated or launched while smask == 0.
    double* scoef = nullptr;         // ssteps x nv x 3 doubles
    int ssteps = 0, snext = 0;       // rows of the table; the row the next step of hf_run_tangent uses
    int scur = -1;                   // the row of the last step taken (-1: none since the table was set or the tangents were reset)
    unsigned smask = 0;              // bit j: column j has a non-zero coefficient in some row
    // derivative tables (hf_tangent_set_tables): per kind a [64][nv] table of offsets into the values (by
    // tag-dictionary index and column, -1 = none).  Nothing is allocated while no entry of the kind is set; k_tangent_load_T<nv>
    // runs exactly while hf_table_derivatives is on.
    int32_t *tkoff = nullptr, *tcoff = nullptr;
    double *tkvals = nullptr, *tcvals = nullptr;
  } tan;
  int fsamp_cap = 0;
  // temperature-dependent conductivities (hf_set_kappa_tables): per row-gather tag-dictionary entry a table header (KTab,
  // n = 0: the constant of d_kappa_rg) and one value array; every step re-values A at the evaluation state (k_assemble_rows_kT)
  // temperature-dependent heat capacities (hf_set_rhoc_tables): a second header array and value array of the same shape; while
  // one is set every evaluation re-values M as well as A (k_assemble_rows_cT).  `on` = tables of either kind are set.
  struct KappaT {
    bool on = false;
    bool k_on = false, c_on = false;   // conductivity tables / capacity tables are set
    int picard = 1;
    KTab* hdr = nullptr;          // 64 entries (all n = 0 while only capacity tables are set)
    double* vals = nullptr;
    std::vector<char> tabled;     // by cell tag: the tag carries a table
    KTab* chdr = nullptr;         // capacity tables: 64 entries
    double* cvals = nullptr;
    std::vector<char> ctabled;    // by cell tag: the tag carries a capacity table
    double* w = nullptr;          // capacity tables, sweeps > 1: the vector the re-valued M multiplies (u^n, or BDF2's operand)
    double *pic = nullptr, *b0 = nullptr;   // evaluation state of the last sweep (for the change), b before lifting (sweeps > 1)
    unsigned long long* change = nullptr;   // max |u^{n+1,p} - u^{n+1,p-1}| of the last step's last sweep (bits of a double >= 0)
    bool have_change = false;
    // hf_table_derivatives: tangent runs of the lagged scheme are allowed; host copies of both header arrays
    // (by tag-dictionary index), which hf_tangent_set_tables sizes its entries by
    bool deriv = false;
    std::vector<KTab> h_hdr, h_chdr;
    // the enthalpy form of the capacity (hf_set_capacity_form).  Nothing below is allocated, launched or read
    // while form == 0 and hf_stored_heat has not been called.
    int form = 0;                    // 0 lagged: rho_c(T_e(x_{k-1})); 1 enthalpy: the chord capacity between u^n and e_{k-1}
    double tol = 0.0, relax = 1.0;   // hf_set_picard_control: stop at change_k <= tol (0: every sweep runs), e += relax (x - e)
    std::vector<double> h_cvals;     // host copy of cvals, from which ccum is built on first use
    double* ccum = nullptr;          // cumulative trapezoids per knot, in knot units: the layout of cvals
    double* e = nullptr;             // the evaluation state e_{k-1}
    unsigned long long* hchange = nullptr;   // change_k of the last sweep of every step since the form was set / the history cleared
    int64_t hcap = 0;
    std::vector<int32_t> hsweeps;    // sweeps of every such step
  } kt;
  // stored heat (hf_stored_heat, hf_set_heat_records): per cell tag sum_e vol_e (H_tag(Tw_e(u)) - H_tag(T_ref))
  struct Heat {
    bool ready = false;              // the buffers below exist (first use)
    int nd = 0, nchunks = 0, grid = 0;   // row-gather dictionary entries; k_monitor's chunks and grid
    uint8_t* slot = nullptr;         // tab_len entries: row-gather dictionary index of a cell tag, 255 = not a cell tag of the mesh
    int32_t* tags = nullptr;         // 64 entries: the cell tag of a dictionary index
    KTab* none = nullptr;            // 64 empty headers, for a context without capacity tables
    double* part = nullptr;          // grid x 64 partials
    double* now = nullptr;           // one record (tab_len doubles), for hf_stored_heat
    bool rec_on = false;
    double T_ref = 0.0;
    double* rec = nullptr;           // cap records of tab_len doubles
    int64_t cap = 0, count = 0;
  } heat;
  // variable time steps (hf_set_step, hf_set_step_list, hf_set_step_control).  The time record (t, h, nh, dt0,
  // dt_eff) is host arithmetic of every step; nothing else below is allocated, launched or read while `on` and `control` are false.
  struct VarStep {
    bool on = false;             // hf_set_step / hf_set_step_list since the last hf_assemble: steps take their size from dt_next / list
    double t = 0.0;              // time of the state since the record was last "at rest"
    double h[3] = {0.0, 0.0, 0.0};   // sizes of the last steps taken, h[0] the newest
    int nh = 0;                  // steps taken since rest
    double dt0 = 0.0;            // size of the first of them (the spacing of the virtual rest states before it)
    double dt_eff = 0.0;         // dt' of the last step taken (ctx->dt is the dt' sys.A holds: the same except after a rejection)
    double dt_next = 0.0;        // hf_set_step: size of the following steps
    std::vector<double> list;    // hf_set_step_list: sizes of the next steps, consumed one per step
    size_t next = 0;
    long long revaluations = 0;  // launches of the assembly kernel for a new dt' (under tables: steps whose dt' differed)
    bool last_changed = false;   // the last step changed the operator ...
    bool carry = false;          // ... and was rejected: its redo, which finds the operator in place, still runs as a step that changed it
    // hf_set_step_control: what an estimate and a rejection need
    bool control = false;
    double *b0 = nullptr, *p1 = nullptr, *p2 = nullptr;   // u^n (copied before the step), u^{n-1}, u^{n-2} (BDF2 only)
    double* s_uprev = nullptr;   // d_uprev as it was before the step
    uint8_t* free_row = nullptr; // 1 on the free rows (k_step_error)
    bool mask_ok = false;
    unsigned long long* err = nullptr;
    bool pending = false;        // a step has been taken under control and neither committed (by the next step) nor rejected
    bool store_pending = false;  // ... and its (solution, right-hand side) pair still has to join the projection ring
    struct Saved {
      double t, h[3], dt0, dt_eff;
      int nh;
      bool bdf_hist, have_prev;
      int g_hist;
      std::vector<double> g0, g1;
      size_t src_next, list_next, resp;
      int64_t mon_count, heat_count;
      int pred_iters, start_kind;
      bool kt_have_change;
    } saved;
  } vs;
  // optional in-situ kernel timing (hf_set_profile): event pairs around each PCG SpMV launch
  bool prof = false;
  std::vector<hipEvent_t> prof_ev;
  int prof_used = 0, prof_base = 0;
  double prof_spmv_ms = 0.0;
  long long prof_spmv_n = 0;
};

namespace {

int fail(hf_ctx* c, int code, const char* fmt, ...);
inline size_t pad16(size_t b) { return (b + 15) & ~static_cast<size_t>(15); }

// a polite spin: the polling threads of concurrent sessions share host cores with the threads that launch kernels
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}

hipError_t copy_sync(hf_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (bytes == 0) return hipSuccess;
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}

int fail(hf_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HF_HIP(call)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return fail(ctx, HF_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

template <typename T>
int dev_alloc(hf_ctx* ctx, T** p, size_t count) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (count == 0) count = 1;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
  if (e != hipSuccess) return fail(ctx, HF_ERR_ALLOC, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
  return HF_OK;
}
#define HF_TRY(expr) do { int rc_ = (expr); if (rc_ != HF_OK) return rc_; } while (0)

// Host<->device copy that is complete on return, issued on the context's own stream (never the legacy
// stream: contexts driven from other host threads must not serialise on it).
hipError_t copy_sync(hf_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);

template <typename T>
void dev_free(T** p) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
}

// Scratch device buffer released on every exit path of the function that owns it.
template <typename T>
struct DevTemp {
  T* p = nullptr;
  ~DevTemp() { dev_free(&p); }
  DevTemp() = default;
  DevTemp(const DevTemp&) = delete;
  DevTemp& operator=(const DevTemp&) = delete;
};

}  // namespace
