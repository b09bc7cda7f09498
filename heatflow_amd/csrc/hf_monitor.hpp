// Part of libheatflow_hip.so (see heatflow_hip.hip): region monitors (hf_set_monitors) - per cell tag the peak and
// the lowest nodal value with their nodes, int r dA, int u r dA and the r-weighted area above a threshold, after every step.
#pragma once
#include "hf_solver.hpp"

namespace {

constexpr int MON_T = 256;        // threads of k_monitor = triangles per chunk
constexpr int MON_ND = 64;        // monitored tags of one table (the monitor dictionary)
constexpr int MON_F = 7;          // fields of a record row: T_max, node_max, T_min, node_min, I0, I1, H
constexpr int MON_FT = 1024;      // threads of k_monitor_final: one per workgroup of k_monitor
constexpr int MON_NONE = 255;     // dictionary index of a tag that is not monitored

// what a workgroup of k_monitor leaves per dictionary index (structure of arrays: part.X[index * workgroups + workgroup])
struct MonPart {
  double *I0, *I1, *H, *vmax, *vmin;
  int32_t *imax, *imin;
};

// The three integrals of one triangle, every operation in the order DESIGN.md 3.17 pins (no contraction):
//   d    = (z1 - z0) (r2 - r0) - (z2 - z0) (r1 - r0),  A = 0.5 |d|,  rs = (r0 + r1) + r2
//   I0   = (A rs) / 3
//   I1   = (A / 12) (((rs + r0) u0 + (rs + r1) u1) + (rs + r2) u2)
//   H    = 0 / I0 with 0 / 3 nodes above theta (u > theta); with one node a above, or one node a not above, b and c the next two
//          in the triangle's order:  sb = (ua - theta) / (ua - ub),  sc = (ua - theta) / (ua - uc),
//          cut = (((A sb) sc) ((ra + (ra + sb (rb - ra))) + (ra + sc (rc - ra)))) / 3;   H = cut (one above) or I0 - cut (two above)
struct MonTerm { double I0, I1, H; };
__device__ __forceinline__ MonTerm monitor_term(const double2 P0, const double2 P1, const double2 P2, double u0, double u1, double u2,
                                                double theta) {
#pragma clang fp contract(off)
  const double d = (P1.x - P0.x) * (P2.y - P0.y) - (P2.x - P0.x) * (P1.y - P0.y);
  const double A = 0.5 * fabs(d);
  const double rs = (P0.y + P1.y) + P2.y;
  MonTerm o;
  o.I0 = (A * rs) / 3.0;
  o.I1 = (A / 12.0) * (((rs + P0.y) * u0 + (rs + P1.y) * u1) + (rs + P2.y) * u2);
  const bool a0 = u0 > theta, a1 = u1 > theta, a2 = u2 > theta;
  const int cnt = static_cast<int>(a0) + static_cast<int>(a1) + static_cast<int>(a2);
  if (cnt == 0) { o.H = 0.0; return o; }
  if (cnt == 3) { o.H = o.I0; return o; }
  // the odd node out: the one above (cnt == 1) or the one not above (cnt == 2)
  const bool odd = cnt == 1;
  const int a = (a0 == odd) ? 0 : (a1 == odd) ? 1 : 2;
  const double ua = a == 0 ? u0 : a == 1 ? u1 : u2, ub = a == 0 ? u1 : a == 1 ? u2 : u0, uc = a == 0 ? u2 : a == 1 ? u0 : u1;
  const double ra = a == 0 ? P0.y : a == 1 ? P1.y : P2.y, rb = a == 0 ? P1.y : a == 1 ? P2.y : P0.y, rc = a == 0 ? P2.y : a == 1 ? P0.y : P1.y;
  const double sb = (ua - theta) / (ua - ub), sc = (ua - theta) / (ua - uc);
  const double cut = (((A * sb) * sc) * ((ra + (ra + sb * (rb - ra))) + (ra + sc * (rc - ra)))) / 3.0;
  o.H = odd ? cut : o.I0 - cut;
  return o;
}

// (value, node) pairs: the larger value wins, among equal values the smaller node (and the mirror image for the minimum) - an
// operation that is associative and commutative, so the result does not depend on the order of the visits
__device__ __forceinline__ void mon_take_max(double& v, int& i, double ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__device__ __forceinline__ void mon_take_min(double& v, int& i, double ov, int oi) {
  if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// One lane per triangle of d_elem, chunks of MON_T triangles dealt to the workgroups by ChunkIter (a schedule of the grid, which
// the mesh alone fixes: min(chunks, MAXP), a multiple of 8 from 64 up).  A lane whose tag is not monitored loads nothing more.  Per
// chunk every wave reduces, for each dictionary index present among its 64 triangles (Morton order: mostly one), the terms of the
// lanes with that index by a shuffle tree and adds the result to the wave's own LDS accumulator - chunk after chunk in ascending
// order, so each accumulator is a fixed sequence of additions.  At the end the four waves' accumulators are added in wave order
// and the workgroup writes its partial of every dictionary index.  No atomics; the bits depend on the mesh, the table and u only.
__global__ __launch_bounds__(MON_T) void k_monitor(int ne, int nchunks, int tab_len, int nd, const int4* __restrict__ elem,
                                                  const double2* __restrict__ zr, const double* __restrict__ u,
                                                  const uint8_t* __restrict__ slot_of_tag, const double* __restrict__ theta, MonPart part) {
  extern __shared__ uint8_t s_slot[];       // tab_len entries: dictionary index of a cell tag, MON_NONE = not monitored
  __shared__ double s_th[MON_ND];
  __shared__ double s_I0[4][MON_ND], s_I1[4][MON_ND], s_H[4][MON_ND], s_vmax[4][MON_ND], s_vmin[4][MON_ND];
  __shared__ int s_imax[4][MON_ND], s_imin[4][MON_ND];
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  for (int i = t; i < tab_len; i += MON_T) s_slot[i] = slot_of_tag[i];
  if (t < MON_ND) s_th[t] = theta[t];
  s_I0[wv][lane] = 0.0; s_I1[wv][lane] = 0.0; s_H[wv][lane] = 0.0;
  s_vmax[wv][lane] = -INFINITY; s_vmin[wv][lane] = INFINITY;
  s_imax[wv][lane] = INT32_MAX; s_imin[wv][lane] = INT32_MAX;
  __syncthreads();
  for (ChunkIter it(nchunks); it.chunk < it.end; it.chunk += it.step) {
    const int e = it.chunk * MON_T + t;
    int d = -1;
    int4 E = make_int4(0, 0, 0, 0);
    if (e < ne) {
      E = elem[e];
      const int s = s_slot[E.w];
      if (s != MON_NONE) d = s;
    }
    MonTerm m{0.0, 0.0, 0.0};
    double vmax = -INFINITY, vmin = INFINITY;
    int imax = INT32_MAX, imin = INT32_MAX;
    if (d >= 0) {
      const double u0 = u[E.x], u1 = u[E.y], u2 = u[E.z];
      m = monitor_term(zr[E.x], zr[E.y], zr[E.z], u0, u1, u2, s_th[d]);
      vmax = u0; imax = E.x; mon_take_max(vmax, imax, u1, E.y); mon_take_max(vmax, imax, u2, E.z);
      vmin = u0; imin = E.x; mon_take_min(vmin, imin, u1, E.y); mon_take_min(vmin, imin, u2, E.z);
    }
    unsigned long long todo = __ballot(d >= 0);      // the same in every lane: the loop is uniform over the wave
    while (todo != 0ull) {
      const int ds = __shfl(d, __ffsll(static_cast<long long>(todo)) - 1, 64);
      const bool mine = d == ds;
      double a0 = mine ? m.I0 : 0.0, a1 = mine ? m.I1 : 0.0, a2 = mine ? m.H : 0.0;
      double bmax = mine ? vmax : -INFINITY, bmin = mine ? vmin : INFINITY;
      int jmax = mine ? imax : INT32_MAX, jmin = mine ? imin : INT32_MAX;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
#pragma clang fp contract(off)
        a0 += __shfl_down(a0, o, 64);
        a1 += __shfl_down(a1, o, 64);
        a2 += __shfl_down(a2, o, 64);
        mon_take_max(bmax, jmax, __shfl_down(bmax, o, 64), __shfl_down(jmax, o, 64));
        mon_take_min(bmin, jmin, __shfl_down(bmin, o, 64), __shfl_down(jmin, o, 64));
      }
      if (lane == 0) {
#pragma clang fp contract(off)
        s_I0[wv][ds] += a0; s_I1[wv][ds] += a1; s_H[wv][ds] += a2;
        double v = s_vmax[wv][ds]; int i = s_imax[wv][ds];
        mon_take_max(v, i, bmax, jmax);
        s_vmax[wv][ds] = v; s_imax[wv][ds] = i;
        v = s_vmin[wv][ds]; i = s_imin[wv][ds];
        mon_take_min(v, i, bmin, jmin);
        s_vmin[wv][ds] = v; s_imin[wv][ds] = i;
      }
      todo &= ~__ballot(mine);
    }
  }
  __syncthreads();
  if (t < nd) {
#pragma clang fp contract(off)
    const size_t o = static_cast<size_t>(t) * gridDim.x + blockIdx.x;
    part.I0[o] = ((s_I0[0][t] + s_I0[1][t]) + s_I0[2][t]) + s_I0[3][t];
    part.I1[o] = ((s_I1[0][t] + s_I1[1][t]) + s_I1[2][t]) + s_I1[3][t];
    part.H[o] = ((s_H[0][t] + s_H[1][t]) + s_H[2][t]) + s_H[3][t];
    double v = s_vmax[0][t], w = s_vmin[0][t];
    int i = s_imax[0][t], j = s_imin[0][t];
    for (int k = 1; k < 4; ++k) {
      mon_take_max(v, i, s_vmax[k][t], s_imax[k][t]);
      mon_take_min(w, j, s_vmin[k][t], s_imin[k][t]);
    }
    part.vmax[o] = v; part.imax[o] = i; part.vmin[o] = w; part.imin[o] = j;
  }
}

// Workgroup d adds the G <= MON_FT partials of dictionary index d - lane g holds workgroup g's, a shuffle tree per wave, then the
// 16 wave results front to back: a fixed order for a given G, which the mesh alone fixes - and writes the seven fields of its tag's
// row.  Workgroup 0 also writes the zero rows of the tags that are not monitored.
__global__ __launch_bounds__(MON_FT) void k_monitor_final(int G, int tab_len, MonPart part, const uint8_t* __restrict__ slot_of_tag,
                                                         const int32_t* __restrict__ tag_of_slot, double* __restrict__ out) {
  __shared__ double s_I0[16], s_I1[16], s_H[16], s_vmax[16], s_vmin[16];
  __shared__ int s_imax[16], s_imin[16];
  const int d = blockIdx.x, t = threadIdx.x, wv = t >> 6, lane = t & 63;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, v = -INFINITY, w = INFINITY;
  int i = INT32_MAX, j = INT32_MAX;
  if (t < G) {
    const size_t o = static_cast<size_t>(d) * G + t;
    a0 = part.I0[o]; a1 = part.I1[o]; a2 = part.H[o];
    v = part.vmax[o]; i = part.imax[o]; w = part.vmin[o]; j = part.imin[o];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma clang fp contract(off)
    a0 += __shfl_down(a0, o, 64);
    a1 += __shfl_down(a1, o, 64);
    a2 += __shfl_down(a2, o, 64);
    mon_take_max(v, i, __shfl_down(v, o, 64), __shfl_down(i, o, 64));
    mon_take_min(w, j, __shfl_down(w, o, 64), __shfl_down(j, o, 64));
  }
  if (lane == 0) { s_I0[wv] = a0; s_I1[wv] = a1; s_H[wv] = a2; s_vmax[wv] = v; s_imax[wv] = i; s_vmin[wv] = w; s_imin[wv] = j; }
  __syncthreads();
  if (t == 0) {
#pragma clang fp contract(off)
    for (int k = 1; k < MON_FT / 64; ++k) {
      a0 += s_I0[k]; a1 += s_I1[k]; a2 += s_H[k];
      mon_take_max(v, i, s_vmax[k], s_imax[k]);
      mon_take_min(w, j, s_vmin[k], s_imin[k]);
    }
    double* row = out + static_cast<size_t>(tag_of_slot[d]) * MON_F;
    row[0] = v; row[1] = static_cast<double>(i); row[2] = w; row[3] = static_cast<double>(j);
    row[4] = a0; row[5] = a1; row[6] = a2;
  }
  if (d == 0)
    for (int k = t; k < tab_len * MON_F; k += MON_FT)
      if (slot_of_tag[k / MON_F] == MON_NONE) out[k] = 0.0;
}
static_assert(MAXP <= MON_FT, "k_monitor_final holds one partial per lane");

// ---- host side --------------------------------------------------------------------------------------------------------------

void monitor_free(hf_ctx* ctx) {
  hf_ctx::Monitor& M = ctx->mon;
  dev_free(&M.slot); dev_free(&M.tags); dev_free(&M.theta); dev_free(&M.part_f); dev_free(&M.part_i); dev_free(&M.rec); dev_free(&M.now);
  M = hf_ctx::Monitor();
}

inline size_t monitor_row(const hf_ctx* ctx) { return static_cast<size_t>(ctx->tab_len) * MON_F; }

// Room for n_more records behind the ones kept: the buffer grows here, before the caller's first launch, never between launches
int monitor_room(hf_ctx* ctx, int64_t n_more) {
  hf_ctx::Monitor& M = ctx->mon;
  if (!M.on || M.count + n_more <= M.cap) return HF_OK;
  const int64_t cap = std::max<int64_t>(M.count + n_more, 2 * M.cap);
  double* grown = nullptr;
  HF_TRY(dev_alloc(ctx, &grown, static_cast<size_t>(cap) * monitor_row(ctx)));
  if (M.count > 0) {
    const hipError_t e = copy_sync(ctx, grown, M.rec, sizeof(double) * static_cast<size_t>(M.count) * monitor_row(ctx), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { dev_free(&grown); return fail(ctx, HF_ERR_HIP, "monitor records: copy failed: %s", hipGetErrorString(e)); }
  }
  dev_free(&M.rec);
  M.rec = grown;
  M.cap = cap;
  return HF_OK;
}

// The two launches of one evaluation of the current state, on the stream, into `out` (tab_len * MON_F doubles on the device)
void monitor_launch(hf_ctx* ctx, double* out) {
  hf_ctx::Monitor& M = ctx->mon;
  const size_t G = static_cast<size_t>(M.grid) * MON_ND;
  MonPart P;
  P.I0 = M.part_f; P.I1 = M.part_f + G; P.H = M.part_f + 2 * G; P.vmax = M.part_f + 3 * G; P.vmin = M.part_f + 4 * G;
  P.imax = M.part_i; P.imin = M.part_i + G;
  hipLaunchKernelGGL(k_monitor, dim3(M.grid), dim3(MON_T), static_cast<size_t>((ctx->tab_len + 15) & ~15), ctx->stream, ctx->ne, M.nchunks,
                     ctx->tab_len, M.nd, ctx->d_elem, ctx->d_zr, ctx->d_u, M.slot, M.theta, P);
  hipLaunchKernelGGL(k_monitor_final, dim3(M.nd), dim3(MON_FT), 0, ctx->stream, M.grid, ctx->tab_len, P, M.slot, M.tags, out);
}

// The record of the step that has just been queued (the caller made room with monitor_room)
inline void monitor_record(hf_ctx* ctx) {
  hf_ctx::Monitor& M = ctx->mon;
  monitor_launch(ctx, M.rec + static_cast<size_t>(M.count) * monitor_row(ctx));
  M.count += 1;
}

}  // namespace
