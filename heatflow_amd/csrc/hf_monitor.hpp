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

// ---- derivatives of the sums in tangent runs (hf_set_monitor_tangents) ----------------------------------------

constexpr int MON_TF = 5;         // fields of a derivative row: dT_max, dT_min, dI0, dI1, dH
constexpr int MON_NS = 4;         // shape slots (hf_tangent_set_shape allows 4 columns with a velocity)
constexpr size_t MON_LDS = 64 * 1024 - 1024;   // dynamic LDS one workgroup of k_monitor_tan may ask for (s_th is static)

// the shape slots of a launch: velocities n x stride interleaved by node, slot s belongs to column col[s]; n = 0: none
struct MonShape { const double* v; int stride, n; int col[MON_NS]; };
// what a workgroup of k_monitor_tan leaves: I1 / H[(index * nv + j) * workgroups + workgroup], I0[(index * 4 + slot) * workgroups + workgroup]
struct MonTanPart { double *I1, *H, *I0; };

// What the columns of one triangle share: monitor_term's quantities, operation for operation, and of a cut triangle the odd node
// out `a` (b, c follow it in the triangle's order), sb, sc, the two differences of u, of r and the bracket
//   G = (ra + (ra + sb (rb - ra))) + (ra + sc (rc - ra))
struct MonGeo {
  double d, A, rs, r0, r1, r2, I0, I1, H;
  double sb, sc, dab, dac, rba, rca, G;
  int a;           // -1: no cut (0 or 3 nodes above)
  bool odd;        // one node above (H = cut); else two (H = I0 - cut)
};
__device__ __forceinline__ MonGeo monitor_geo(const double2 P0, const double2 P1, const double2 P2, double u0, double u1, double u2,
                                              double theta) {
#pragma clang fp contract(off)
  MonGeo g;
  g.d = (P1.x - P0.x) * (P2.y - P0.y) - (P2.x - P0.x) * (P1.y - P0.y);
  g.A = 0.5 * fabs(g.d);
  g.r0 = P0.y; g.r1 = P1.y; g.r2 = P2.y;
  g.rs = (P0.y + P1.y) + P2.y;
  g.I0 = (g.A * g.rs) / 3.0;
  g.I1 = (g.A / 12.0) * (((g.rs + P0.y) * u0 + (g.rs + P1.y) * u1) + (g.rs + P2.y) * u2);
  g.a = -1; g.odd = false;
  g.sb = g.sc = g.dab = g.dac = g.rba = g.rca = g.G = 0.0;
  const bool a0 = u0 > theta, a1 = u1 > theta, a2 = u2 > theta;
  const int cnt = static_cast<int>(a0) + static_cast<int>(a1) + static_cast<int>(a2);
  if (cnt == 0) { g.H = 0.0; return g; }
  if (cnt == 3) { g.H = g.I0; return g; }
  g.odd = cnt == 1;
  const int a = (a0 == g.odd) ? 0 : (a1 == g.odd) ? 1 : 2;
  g.a = a;
  const double ua = a == 0 ? u0 : a == 1 ? u1 : u2, ub = a == 0 ? u1 : a == 1 ? u2 : u0, uc = a == 0 ? u2 : a == 1 ? u0 : u1;
  const double ra = a == 0 ? P0.y : a == 1 ? P1.y : P2.y, rb = a == 0 ? P1.y : a == 1 ? P2.y : P0.y, rc = a == 0 ? P2.y : a == 1 ? P0.y : P1.y;
  g.dab = ua - ub; g.dac = ua - uc;
  g.sb = (ua - theta) / g.dab; g.sc = (ua - theta) / g.dac;
  g.rba = rb - ra; g.rca = rc - ra;
  g.G = (ra + (ra + g.sb * g.rba)) + (ra + g.sc * g.rca);
  const double cut = (((g.A * g.sb) * g.sc) * g.G) / 3.0;
  g.H = g.odd ? cut : g.I0 - cut;
  return g;
}

// The derivatives of one triangle's I1 and H along one tangent column with nodal values t0, t1, t2 (u moves, the nodes do not),
// every operation in the order DESIGN.md 3.18 pins (no contraction):
//   J1   = (A / 12) (((rs + r0) t0 + (rs + r1) t1) + (rs + r2) t2)
//   pb   = ((1 - sb) ta + sb tb) / (ua - ub),   pc = ((1 - sc) ta + sc tc) / (ua - uc)
//   dcut = (A ((pb sc + sb pc) G + (sb sc) (pb (rb - ra) + pc (rc - ra)))) / 3;   dH = dcut (one above), -dcut (two above), else 0
struct MonTan { double dI1, dH; };
__device__ __forceinline__ MonTan monitor_term_tan(const MonGeo& g, double t0, double t1, double t2) {
#pragma clang fp contract(off)
  MonTan o;
  o.dI1 = (g.A / 12.0) * (((g.rs + g.r0) * t0 + (g.rs + g.r1) * t1) + (g.rs + g.r2) * t2);
  o.dH = 0.0;
  if (g.a >= 0) {
    const int a = g.a;
    const double ta = a == 0 ? t0 : a == 1 ? t1 : t2, tb = a == 0 ? t1 : a == 1 ? t2 : t0, tc = a == 0 ? t2 : a == 1 ? t0 : t1;
    const double pb = ((1.0 - g.sb) * ta + g.sb * tb) / g.dab;
    const double pc = ((1.0 - g.sc) * ta + g.sc * tc) / g.dac;
    const double dcut = (g.A * ((pb * g.sc + g.sb * pc) * g.G + (g.sb * g.sc) * (pb * g.rba + pc * g.rca))) / 3.0;
    o.dH = g.odd ? dcut : -dcut;
  }
  return o;
}

// k_monitor's sibling for the derivatives: one lane per triangle, the same chunks, schedule, slot table and per-wave shuffle trees;
// the lane loads its three nodes' NV tangents s[node * nvt + j0 .. + NV) as vectors, forms (dI1, dH) of every column and, per
// shape slot, q = dd / d with dd = (v1 - v0) (r2 - r0) - (v2 - v0) (r1 - r0): dI0 = q I0 of the slot, and the slot's column gets
// dI1 = J1 + q I1, dH = dH + q H.  The per-wave LDS accumulators - [wave][index][NV] for dI1 and dH, [wave][index][4] for dI0, sized
// by the nd monitored - take one addition per chunk and index present, in ascending chunk order, and are added in wave order at the
// end.  No atomics; the bits of column j depend on the mesh, the table, u, column j of s and the velocities only.
template <int NV>
__global__ __launch_bounds__(MON_T) void k_monitor_tan(int ne, int nchunks, int tab_len, int nd, int nvt, int j0, const int4* __restrict__ elem,
                                                      const double2* __restrict__ zr, const double* __restrict__ u,
                                                      const double* __restrict__ s, const uint8_t* __restrict__ slot_of_tag,
                                                      const double* __restrict__ theta, MonShape sh, MonTanPart part) {
  extern __shared__ double s_acc[];         // 4 x nd x NV (dI1), 4 x nd x NV (dH), 4 x nd x 4 (dI0), then tab_len bytes of slots
  __shared__ double s_th[MON_ND];
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  const int nacc = 4 * nd * (2 * NV + MON_NS);
  double* const s_I1 = s_acc;
  double* const s_H = s_acc + 4 * nd * NV;
  double* const s_I0 = s_acc + 8 * nd * NV;
  uint8_t* const s_slot = reinterpret_cast<uint8_t*>(s_acc + nacc);
  for (int i = t; i < tab_len; i += MON_T) s_slot[i] = slot_of_tag[i];
  if (t < MON_ND) s_th[t] = theta[t];
  for (int i = t; i < nacc; i += MON_T) s_acc[i] = 0.0;
  __syncthreads();
  for (ChunkIter it(nchunks); it.chunk < it.end; it.chunk += it.step) {
    const int e = it.chunk * MON_T + t;
    int d = -1;
    int4 E = make_int4(0, 0, 0, 0);
    if (e < ne) {
      E = elem[e];
      const int sl = s_slot[E.w];
      if (sl != MON_NONE) d = sl;
    }
    double m1[NV], mH[NV], m0[MON_NS];
#pragma unroll
    for (int j = 0; j < NV; ++j) { m1[j] = 0.0; mH[j] = 0.0; }
#pragma unroll
    for (int q = 0; q < MON_NS; ++q) m0[q] = 0.0;
    if (d >= 0) {
#pragma clang fp contract(off)
      const MonGeo g = monitor_geo(zr[E.x], zr[E.y], zr[E.z], u[E.x], u[E.y], u[E.z], s_th[d]);
      const double2* const s0 = reinterpret_cast<const double2*>(s + static_cast<size_t>(E.x) * nvt + j0);
      const double2* const s1 = reinterpret_cast<const double2*>(s + static_cast<size_t>(E.y) * nvt + j0);
      const double2* const s2 = reinterpret_cast<const double2*>(s + static_cast<size_t>(E.z) * nvt + j0);
      double qs[MON_NS];
#pragma unroll
      for (int q = 0; q < MON_NS; ++q) {
        qs[q] = 0.0;
        if (q < sh.n) {
          const double v0 = sh.v[static_cast<size_t>(E.x) * sh.stride + q], v1 = sh.v[static_cast<size_t>(E.y) * sh.stride + q],
                       v2 = sh.v[static_cast<size_t>(E.z) * sh.stride + q];
          const double dd = (v1 - v0) * (g.r2 - g.r0) - (v2 - v0) * (g.r1 - g.r0);
          qs[q] = dd / g.d;
          m0[q] = qs[q] * g.I0;
        }
      }
#pragma unroll
      for (int jj = 0; jj < NV / 2; ++jj) {
        const double2 a = s0[jj], b = s1[jj], c = s2[jj];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int j = 2 * jj + h;
          const MonTan m = monitor_term_tan(g, h ? a.y : a.x, h ? b.y : b.x, h ? c.y : c.x);
          m1[j] = m.dI1; mH[j] = m.dH;
#pragma unroll
          for (int q = 0; q < MON_NS; ++q)
            if (q < sh.n && sh.col[q] == j0 + j) { m1[j] = m1[j] + qs[q] * g.I1; mH[j] = mH[j] + qs[q] * g.H; }
        }
      }
    }
    unsigned long long todo = __ballot(d >= 0);      // the same in every lane: the loop is uniform over the wave
    while (todo != 0ull) {
      const int ds = __shfl(d, __ffsll(static_cast<long long>(todo)) - 1, 64);
      const bool mine = d == ds;
      double* const w1 = s_I1 + (wv * nd + ds) * NV;
      double* const wH = s_H + (wv * nd + ds) * NV;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
#pragma clang fp contract(off)
        double a1 = mine ? m1[j] : 0.0, a2 = mine ? mH[j] : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          a1 += __shfl_down(a1, o, 64);
          a2 += __shfl_down(a2, o, 64);
        }
        if (lane == 0) { w1[j] += a1; wH[j] += a2; }
      }
#pragma unroll
      for (int q = 0; q < MON_NS; ++q) {
#pragma clang fp contract(off)
        if (q < sh.n) {
          double a0 = mine ? m0[q] : 0.0;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) a0 += __shfl_down(a0, o, 64);
          if (lane == 0) s_I0[(wv * nd + ds) * MON_NS + q] += a0;
        }
      }
      todo &= ~__ballot(mine);
    }
  }
  __syncthreads();
  const size_t G = gridDim.x;
  for (int i = t; i < nd * NV; i += MON_T) {
#pragma clang fp contract(off)
    const int dd = i / NV, j = i - dd * NV;
    const size_t o = (static_cast<size_t>(dd) * nvt + j0 + j) * G + blockIdx.x;
    const int w = nd * NV;
    part.I1[o] = ((s_I1[i] + s_I1[w + i]) + s_I1[2 * w + i]) + s_I1[3 * w + i];
    part.H[o] = ((s_H[i] + s_H[w + i]) + s_H[2 * w + i]) + s_H[3 * w + i];
  }
  if (j0 == 0)
    for (int i = t; i < nd * MON_NS; i += MON_T) {
#pragma clang fp contract(off)
      const int w = nd * MON_NS;
      part.I0[static_cast<size_t>(i) * G + blockIdx.x] = ((s_I0[i] + s_I0[w + i]) + s_I0[2 * w + i]) + s_I0[3 * w + i];
    }
}

// Workgroup (d, j) adds the G <= MON_FT partials of dictionary index d and column j as k_monitor_final does (lane g holds workgroup
// g's, a shuffle tree per wave, then the 16 wave results front to back), gathers s_j at the nodes of the extremes, whose ids it
// reads from the primal row of the same state, and writes the five fields of out[(tag * nvt + j) * 5 ..].  Workgroup (0, 0) also
// writes the zero rows of the tags that are not monitored.
__global__ __launch_bounds__(MON_FT) void k_monitor_tan_final(int G, int tab_len, int n, int nvt, MonTanPart part, MonShape sh,
                                                             const double* __restrict__ s, const double* __restrict__ prim,
                                                             const uint8_t* __restrict__ slot_of_tag, const int32_t* __restrict__ tag_of_slot,
                                                             double* __restrict__ out) {
  __shared__ double s_I0[16], s_I1[16], s_H[16];
  const int d = blockIdx.x, j = blockIdx.y, t = threadIdx.x, wv = t >> 6, lane = t & 63;
  int slot = -1;
  for (int q = 0; q < MON_NS; ++q)
    if (q < sh.n && sh.col[q] == j) slot = q;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  if (t < G) {
    const size_t o = (static_cast<size_t>(d) * nvt + j) * G + t;
    a1 = part.I1[o]; a2 = part.H[o];
    if (slot >= 0) a0 = part.I0[(static_cast<size_t>(d) * MON_NS + slot) * G + t];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma clang fp contract(off)
    a0 += __shfl_down(a0, o, 64);
    a1 += __shfl_down(a1, o, 64);
    a2 += __shfl_down(a2, o, 64);
  }
  if (lane == 0) { s_I0[wv] = a0; s_I1[wv] = a1; s_H[wv] = a2; }
  __syncthreads();
  if (t == 0) {
#pragma clang fp contract(off)
    for (int k = 1; k < MON_FT / 64; ++k) { a0 += s_I0[k]; a1 += s_I1[k]; a2 += s_H[k]; }
    const int tag = tag_of_slot[d];
    const double* p = prim + static_cast<size_t>(tag) * MON_F;
    const int imax = static_cast<int>(p[1]), imin = static_cast<int>(p[3]);
    double* row = out + (static_cast<size_t>(tag) * nvt + j) * MON_TF;
    row[0] = imax >= 0 && imax < n ? s[static_cast<size_t>(imax) * nvt + j] : 0.0;
    row[1] = imin >= 0 && imin < n ? s[static_cast<size_t>(imin) * nvt + j] : 0.0;
    row[2] = a0; row[3] = a1; row[4] = a2;
  }
  if (d == 0 && j == 0) {
    const int per = nvt * MON_TF;
    for (int k = t; k < tab_len * per; k += MON_FT)
      if (slot_of_tag[k / per] == MON_NONE) out[k] = 0.0;
  }
}

// ---- records of a batched sweep (hf_batch_set_monitors) ----------------------------------------------------------

// what a workgroup of kb_monitor leaves: I0[index * workgroups + workgroup] (the columns share it) and, per column,
// X[(index * nvt + j) * workgroups + workgroup]
struct MonBPart {
  double *I0, *I1, *H, *vmax, *vmin;
  int32_t *imax, *imin;
};

// k_monitor's sibling for the interleaved state u[node * nvt + j] of a batch: one lane per triangle, the same chunks, ChunkIter
// schedule, slot table and thresholds.  The lane loads its three nodes' NV values u[node * nvt + j0 .. + NV) as vectors and runs
// k_monitor's body once per column: monitor_term on the column's three values (its I0 does not depend on them and is reduced once
// per triangle, for the launch with j0 = 0), the extremes by mon_take_max / mon_take_min, per dictionary index present in the wave
// the same masked shuffle tree, one addition per chunk to the wave's LDS accumulator [wave][index][column] in ascending chunk
// order, the four waves added in wave order at the end.  Every accumulator of column j therefore sees the sequence of operations
// k_monitor's sees for the field u[. * nvt + j]: the same bits.  No atomics.
template <int NV>
__global__ __launch_bounds__(MON_T) void kb_monitor(int ne, int nchunks, int tab_len, int nd, int nvt, int j0, const int4* __restrict__ elem,
                                                   const double2* __restrict__ zr, const double* __restrict__ u,
                                                   const uint8_t* __restrict__ slot_of_tag, const double* __restrict__ theta, MonBPart part) {
  extern __shared__ double s_acc[];         // 4 x [4][nd][NV] doubles (I1, H, vmax, vmin), [4][nd] (I0), 2 x [4][nd][NV] ints, then the slots
  __shared__ double s_th[MON_ND];
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  const int W = 4 * nd * NV;                // entries of one per-column accumulator array
  double* const s_I1 = s_acc;
  double* const s_H = s_acc + W;
  double* const s_vmax = s_acc + 2 * W;
  double* const s_vmin = s_acc + 3 * W;
  double* const s_I0 = s_acc + 4 * W;
  int* const s_imax = reinterpret_cast<int*>(s_I0 + 4 * nd);
  int* const s_imin = s_imax + W;
  uint8_t* const s_slot = reinterpret_cast<uint8_t*>(s_imin + W);
  for (int i = t; i < tab_len; i += MON_T) s_slot[i] = slot_of_tag[i];
  if (t < MON_ND) s_th[t] = theta[t];
  for (int i = t; i < W; i += MON_T) {
    s_I1[i] = 0.0; s_H[i] = 0.0; s_vmax[i] = -INFINITY; s_vmin[i] = INFINITY;
    s_imax[i] = INT32_MAX; s_imin[i] = INT32_MAX;
  }
  for (int i = t; i < 4 * nd; i += MON_T) s_I0[i] = 0.0;
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
    double2 P0 = make_double2(0.0, 0.0), P1 = P0, P2 = P0;
    double th = 0.0;
    const double2 *q0 = nullptr, *q1 = nullptr, *q2 = nullptr;
    if (d >= 0) {
      P0 = zr[E.x]; P1 = zr[E.y]; P2 = zr[E.z];
      th = s_th[d];
      q0 = reinterpret_cast<const double2*>(u + static_cast<size_t>(E.x) * nvt + j0);
      q1 = reinterpret_cast<const double2*>(u + static_cast<size_t>(E.y) * nvt + j0);
      q2 = reinterpret_cast<const double2*>(u + static_cast<size_t>(E.z) * nvt + j0);
    }
    const unsigned long long present = __ballot(d >= 0);      // the same in every lane: the loops below are uniform over the wave
#pragma unroll
    for (int jj = 0; jj < NV / 2; ++jj) {
      double2 a = make_double2(0.0, 0.0), b = a, c = a;
      if (d >= 0) { a = q0[jj]; b = q1[jj]; c = q2[jj]; }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int j = 2 * jj + h;
        MonTerm m{0.0, 0.0, 0.0};
        double vmax = -INFINITY, vmin = INFINITY;
        int imax = INT32_MAX, imin = INT32_MAX;
        if (d >= 0) {
          const double u0 = h ? a.y : a.x, u1 = h ? b.y : b.x, u2 = h ? c.y : c.x;
          m = monitor_term(P0, P1, P2, u0, u1, u2, th);
          vmax = u0; imax = E.x; mon_take_max(vmax, imax, u1, E.y); mon_take_max(vmax, imax, u2, E.z);
          vmin = u0; imin = E.x; mon_take_min(vmin, imin, u1, E.y); mon_take_min(vmin, imin, u2, E.z);
        }
        const bool with_I0 = j == 0 && j0 == 0;              // I0 of the triangle: reduced with the first column of the first group
        unsigned long long todo = present;
        while (todo != 0ull) {
          const int ds = __shfl(d, __ffsll(static_cast<long long>(todo)) - 1, 64);
          const bool mine = d == ds;
          double a0 = mine ? m.I0 : 0.0, a1 = mine ? m.I1 : 0.0, a2 = mine ? m.H : 0.0;
          double bmax = mine ? vmax : -INFINITY, bmin = mine ? vmin : INFINITY;
          int jmax = mine ? imax : INT32_MAX, jmin = mine ? imin : INT32_MAX;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
#pragma clang fp contract(off)
            if (with_I0) a0 += __shfl_down(a0, o, 64);
            a1 += __shfl_down(a1, o, 64);
            a2 += __shfl_down(a2, o, 64);
            mon_take_max(bmax, jmax, __shfl_down(bmax, o, 64), __shfl_down(jmax, o, 64));
            mon_take_min(bmin, jmin, __shfl_down(bmin, o, 64), __shfl_down(jmin, o, 64));
          }
          if (lane == 0) {
#pragma clang fp contract(off)
            const int k = (wv * nd + ds) * NV + j;
            if (with_I0) s_I0[wv * nd + ds] += a0;
            s_I1[k] += a1; s_H[k] += a2;
            double v = s_vmax[k]; int i = s_imax[k];
            mon_take_max(v, i, bmax, jmax);
            s_vmax[k] = v; s_imax[k] = i;
            v = s_vmin[k]; i = s_imin[k];
            mon_take_min(v, i, bmin, jmin);
            s_vmin[k] = v; s_imin[k] = i;
          }
          todo &= ~__ballot(mine);
        }
      }
    }
  }
  __syncthreads();
  const size_t G = gridDim.x;
  const int w = nd * NV;
  for (int i = t; i < w; i += MON_T) {
#pragma clang fp contract(off)
    const int dd = i / NV, j = i - dd * NV;
    const size_t o = (static_cast<size_t>(dd) * nvt + j0 + j) * G + blockIdx.x;
    part.I1[o] = ((s_I1[i] + s_I1[w + i]) + s_I1[2 * w + i]) + s_I1[3 * w + i];
    part.H[o] = ((s_H[i] + s_H[w + i]) + s_H[2 * w + i]) + s_H[3 * w + i];
    double v = s_vmax[i], x = s_vmin[i];
    int p = s_imax[i], q = s_imin[i];
    for (int k = 1; k < 4; ++k) {
      mon_take_max(v, p, s_vmax[k * w + i], s_imax[k * w + i]);
      mon_take_min(x, q, s_vmin[k * w + i], s_imin[k * w + i]);
    }
    part.vmax[o] = v; part.imax[o] = p; part.vmin[o] = x; part.imin[o] = q;
  }
  if (j0 == 0)
    for (int i = t; i < nd; i += MON_T) {
#pragma clang fp contract(off)
      part.I0[static_cast<size_t>(i) * G + blockIdx.x] = ((s_I0[i] + s_I0[nd + i]) + s_I0[2 * nd + i]) + s_I0[3 * nd + i];
    }
}

// Workgroup (d, j) adds the G <= MON_FT partials of dictionary index d and column j exactly as k_monitor_final adds those of d
// (lane g holds workgroup g's, a shuffle tree per wave, then the 16 wave results front to back) and writes the seven fields of
// out[(j * tab_len + tag) * 7 ..].  Workgroup (0, j) also writes the zero rows of column j's tags that are not monitored.
__global__ __launch_bounds__(MON_FT) void kb_monitor_final(int G, int tab_len, int nvt, MonBPart part, const uint8_t* __restrict__ slot_of_tag,
                                                          const int32_t* __restrict__ tag_of_slot, double* __restrict__ out) {
  __shared__ double s_I0[16], s_I1[16], s_H[16], s_vmax[16], s_vmin[16];
  __shared__ int s_imax[16], s_imin[16];
  const int d = blockIdx.x, jc = blockIdx.y, t = threadIdx.x, wv = t >> 6, lane = t & 63;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, v = -INFINITY, w = INFINITY;
  int i = INT32_MAX, j = INT32_MAX;
  if (t < G) {
    const size_t o = (static_cast<size_t>(d) * nvt + jc) * G + t;
    a0 = part.I0[static_cast<size_t>(d) * G + t]; a1 = part.I1[o]; a2 = part.H[o];
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
  double* const col = out + static_cast<size_t>(jc) * tab_len * MON_F;
  if (t == 0) {
#pragma clang fp contract(off)
    for (int k = 1; k < MON_FT / 64; ++k) {
      a0 += s_I0[k]; a1 += s_I1[k]; a2 += s_H[k];
      mon_take_max(v, i, s_vmax[k], s_imax[k]);
      mon_take_min(w, j, s_vmin[k], s_imin[k]);
    }
    double* row = col + static_cast<size_t>(tag_of_slot[d]) * MON_F;
    row[0] = v; row[1] = static_cast<double>(i); row[2] = w; row[3] = static_cast<double>(j);
    row[4] = a0; row[5] = a1; row[6] = a2;
  }
  if (d == 0)
    for (int k = t; k < tab_len * MON_F; k += MON_FT)
      if (slot_of_tag[k / MON_F] == MON_NONE) col[k] = 0.0;
}

// ---- host side --------------------------------------------------------------------------------------------------------------

void monitor_free(hf_ctx* ctx) {
  hf_ctx::Monitor& M = ctx->mon;
  dev_free(&M.slot); dev_free(&M.tags); dev_free(&M.theta); dev_free(&M.part_f); dev_free(&M.part_i); dev_free(&M.rec); dev_free(&M.now);
  dev_free(&M.tpart); dev_free(&M.trec);
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

// ---- derivative records ---------------------------------------------------------------------------------------

inline size_t montan_row(const hf_ctx* ctx, int nv) { return static_cast<size_t>(ctx->tab_len) * nv * MON_TF; }

// dynamic LDS of k_monitor_tan<NV>: the accumulators of the nd monitored tags, then the slot table
inline size_t montan_lds(const hf_ctx* ctx, int NV) {
  return sizeof(double) * 4 * ctx->mon.nd * (2 * NV + MON_NS) + static_cast<size_t>((ctx->tab_len + 15) & ~15);
}

// The partials of k_monitor_tan, for the widest nv: allocated by hf_set_monitor_tangents(1) or the first hf_monitor_tangent_eval
int montan_parts(hf_ctx* ctx) {
  hf_ctx::Monitor& M = ctx->mon;
  if (M.tpart) return HF_OK;
  return dev_alloc(ctx, &M.tpart, static_cast<size_t>(M.nd) * (2 * NV_MAX + MON_NS) * M.grid);
}

// Drop the derivative records (the buffer goes too: its rows belong to one nv)
void montan_drop(hf_ctx* ctx) {
  hf_ctx::Monitor& M = ctx->mon;
  dev_free(&M.trec);
  M.tcap = 0; M.tcount = 0; M.tnv = 0;
  M.tindex.clear();
}

// Room for n_more derivative records of nv columns behind the ones kept, before the caller's first launch (as monitor_room)
int montan_room(hf_ctx* ctx, int nv, int64_t n_more) {
  hf_ctx::Monitor& M = ctx->mon;
  if (!M.on || !M.tan_on) return HF_OK;
  if (M.tnv != nv) { montan_drop(ctx); M.tnv = nv; }
  M.tindex.reserve(static_cast<size_t>(M.tcount + n_more));
  if (M.tcount + n_more <= M.tcap) return HF_OK;
  const int64_t cap = std::max<int64_t>(M.tcount + n_more, 2 * M.tcap);
  double* grown = nullptr;
  HF_TRY(dev_alloc(ctx, &grown, static_cast<size_t>(cap) * montan_row(ctx, nv)));
  if (M.tcount > 0) {
    const hipError_t e = copy_sync(ctx, grown, M.trec, sizeof(double) * static_cast<size_t>(M.tcount) * montan_row(ctx, nv), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { dev_free(&grown); return fail(ctx, HF_ERR_HIP, "monitor derivative records: copy failed: %s", hipGetErrorString(e)); }
  }
  dev_free(&M.trec);
  M.trec = grown;
  M.tcap = cap;
  return HF_OK;
}

// The launches of one derivative row on the stream: tangents `s` (n x nv interleaved) of the state in ctx->d_u, whose primal row is
// `prim`, into `out` (tab_len x nv x 5 doubles on the device).  The columns go in one launch where its accumulators fit the LDS
// of a workgroup, else in groups of the widest power of two that does (a function of nd and nv alone), one launch per group.
void montan_launch(hf_ctx* ctx, int nv, const double* s, const MonShape& sh, const double* prim, double* out) {
  hf_ctx::Monitor& M = ctx->mon;
  const size_t G = static_cast<size_t>(M.grid) * M.nd;
  MonTanPart P;
  P.I1 = M.tpart; P.H = M.tpart + G * NV_MAX; P.I0 = M.tpart + 2 * G * NV_MAX;
  int gw = nv;
  while (gw > 2 && montan_lds(ctx, gw) > MON_LDS) gw >>= 1;
  const size_t sm = montan_lds(ctx, gw);
  for (int j0 = 0; j0 < nv; j0 += gw)
    dispatch_nv(gw, [&](auto w) {
      hipLaunchKernelGGL(k_monitor_tan<decltype(w)::value>, dim3(M.grid), dim3(MON_T), sm, ctx->stream, ctx->ne, M.nchunks, ctx->tab_len,
                         M.nd, nv, j0, ctx->d_elem, ctx->d_zr, ctx->d_u, s, M.slot, M.theta, sh, P);
    });
  hipLaunchKernelGGL(k_monitor_tan_final, dim3(M.nd, nv), dim3(MON_FT), 0, ctx->stream, M.grid, ctx->tab_len, ctx->n, nv, P, sh, s, prim, M.slot,
                     M.tags, out);
}

// The derivative record of the step whose primal record was taken last (the caller made room with montan_room)
inline void montan_record(hf_ctx* ctx) {
  hf_ctx::Monitor& M = ctx->mon;
  const hf_ctx::Tangent::Shape& S = ctx->tan.sh;
  MonShape sh{S.d_v, S.ns, S.ncol, {S.col[0], S.col[1], S.col[2], S.col[3]}};
  montan_launch(ctx, M.tnv, ctx->tanb.u, sh, M.rec + static_cast<size_t>(M.count - 1) * monitor_row(ctx),
                M.trec + static_cast<size_t>(M.tcount) * montan_row(ctx, M.tnv));
  M.tindex.push_back(static_cast<int32_t>(M.count - 1));
  M.tcount += 1;
}

// ---- records of the open batch -----------------------------------------------------------------------------------

inline size_t bmon_row(const hf_ctx* ctx) { return static_cast<size_t>(ctx->batch.nv) * monitor_row(ctx); }

// dynamic LDS of kb_monitor<NV>: per wave and monitored tag four doubles and two ints per column and one double (I0), then the slots
inline size_t bmon_lds(const hf_ctx* ctx, int NV) {
  return static_cast<size_t>(4) * ctx->mon.nd * (static_cast<size_t>(NV) * (4 * sizeof(double) + 2 * sizeof(int)) + sizeof(double)) +
         static_cast<size_t>((ctx->tab_len + 15) & ~15);
}

// Room for n_more records of the open batch behind the ones kept, before the caller's first launch (as monitor_room)
int bmon_room(hf_ctx* ctx, int64_t n_more) {
  hf_ctx::BatchMonitor& M = ctx->bmon;
  if (!M.on || M.count + n_more <= M.cap) return HF_OK;
  const int64_t cap = std::max<int64_t>(M.count + n_more, 2 * M.cap);
  double* grown = nullptr;
  HF_TRY(dev_alloc(ctx, &grown, static_cast<size_t>(cap) * bmon_row(ctx)));
  if (M.count > 0) {
    const hipError_t e = copy_sync(ctx, grown, M.rec, sizeof(double) * static_cast<size_t>(M.count) * bmon_row(ctx), hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { dev_free(&grown); return fail(ctx, HF_ERR_HIP, "batch monitor records: copy failed: %s", hipGetErrorString(e)); }
  }
  dev_free(&M.rec);
  M.rec = grown;
  M.cap = cap;
  return HF_OK;
}

// The launches of one evaluation of the open batch's state, on the stream, into `out` (nv x tab_len x MON_F doubles on the device).
// The columns go in one launch where its accumulators fit the LDS of a workgroup, else in groups of the widest power of two that
// does (a function of nd and nv alone), one launch per group, as montan_launch does.
void bmon_launch(hf_ctx* ctx, double* out) {
  const hf_ctx::Monitor& M = ctx->mon;
  const hf_ctx::BatchMonitor& Q = ctx->bmon;
  const int nv = ctx->batch.nv;
  const size_t G = static_cast<size_t>(M.grid) * M.nd, GV = G * nv;
  MonBPart P;
  P.I0 = Q.part_f; P.I1 = Q.part_f + G; P.H = P.I1 + GV; P.vmax = P.H + GV; P.vmin = P.vmax + GV;
  P.imax = Q.part_i; P.imin = Q.part_i + GV;
  int gw = nv;
  while (gw > 2 && bmon_lds(ctx, gw) > MON_LDS) gw >>= 1;
  const size_t sm = bmon_lds(ctx, gw);
  for (int j0 = 0; j0 < nv; j0 += gw)
    dispatch_nv(gw, [&](auto w) {
      hipLaunchKernelGGL(kb_monitor<decltype(w)::value>, dim3(M.grid), dim3(MON_T), sm, ctx->stream, ctx->ne, M.nchunks, ctx->tab_len, M.nd,
                         nv, j0, ctx->d_elem, ctx->d_zr, ctx->batch.u, M.slot, M.theta, P);
    });
  hipLaunchKernelGGL(kb_monitor_final, dim3(M.nd, nv), dim3(MON_FT), 0, ctx->stream, M.grid, ctx->tab_len, nv, P, M.slot, M.tags, out);
}

// The record of the batched step that has just been queued (the caller made room with bmon_room)
inline void bmon_record(hf_ctx* ctx) {
  hf_ctx::BatchMonitor& M = ctx->bmon;
  bmon_launch(ctx, M.rec + static_cast<size_t>(M.count) * bmon_row(ctx));
  M.count += 1;
}

// ---- stored heat (hf_stored_heat, hf_set_heat_records) -----------------------------------------------------------

// Per cell tag sum_e vol_e (H_tag(Tw_e(u)) - H_tag(T_ref)), vol_e = (A_e rs) / 3 as k_monitor's I0, Tw_e the r-weighted element
// temperature of the assembly (element_tw) and H_tag the integral of the tag's clamped capacity table - formed without a
// difference of two integrals as mean(T_ref, Tw_e) (Tw_e - T_ref) (ktab_mean) - or rho_c T of a tag without one.  k_monitor's
// reduction with one accumulator: one lane per triangle, the same chunks and schedule, per-wave shuffle trees into per-wave LDS
// accumulators in ascending chunk order, the four waves added in wave order.  The dictionary is the row-gather tag dictionary
// (every cell tag of the mesh).  No atomics; the bits depend on the mesh, the tables, T_ref and u only.
__global__ __launch_bounds__(MON_T) void k_stored_heat(int ne, int nchunks, int tab_len, int nd, const int4* __restrict__ elem,
                                                      const double2* __restrict__ zr, const double* __restrict__ u,
                                                      const uint8_t* __restrict__ slot_of_tag, const KTab* __restrict__ ctab,
                                                      const double* __restrict__ cvals, const double* __restrict__ ccum,
                                                      const double* __restrict__ rhoc_idx, double T_ref, double* __restrict__ part) {
  extern __shared__ uint8_t s_slot[];       // tab_len entries: dictionary index of a cell tag
  __shared__ KTab s_ct[MON_ND];
  __shared__ double s_rc[MON_ND];
  __shared__ double s_E[4][MON_ND];
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63;
  for (int i = t; i < tab_len; i += MON_T) s_slot[i] = slot_of_tag[i];
  if (t < MON_ND) { s_ct[t] = ctab[t]; s_rc[t] = rhoc_idx[t]; }
  s_E[wv][lane] = 0.0;
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
    double m = 0.0;
    if (d >= 0) {
#pragma clang fp contract(off)
      const double2 P0 = zr[E.x], P1 = zr[E.y], P2 = zr[E.z];
      const double dd = (P1.x - P0.x) * (P2.y - P0.y) - (P2.x - P0.x) * (P1.y - P0.y);
      const double vol = ((0.5 * fabs(dd)) * ((P0.y + P1.y) + P2.y)) / 3.0;
      const double Tw = element_tw(P0.y, P1.y, P2.y, u[E.x], u[E.y], u[E.z]);
      const KTab ch = s_ct[d];
      const double c = ch.n > 0 ? ktab_mean(ch, cvals, ccum, T_ref, Tw) : s_rc[d];
      m = vol * (c * (Tw - T_ref));
    }
    unsigned long long todo = __ballot(d >= 0);      // the same in every lane: the loop is uniform over the wave
    while (todo != 0ull) {
      const int ds = __shfl(d, __ffsll(static_cast<long long>(todo)) - 1, 64);
      const bool mine = d == ds;
      double a = mine ? m : 0.0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
#pragma clang fp contract(off)
        a += __shfl_down(a, o, 64);
      }
      if (lane == 0) {
#pragma clang fp contract(off)
        s_E[wv][ds] += a;
      }
      todo &= ~__ballot(mine);
    }
  }
  __syncthreads();
  if (t < nd) {
#pragma clang fp contract(off)
    part[static_cast<size_t>(t) * gridDim.x + blockIdx.x] = ((s_E[0][t] + s_E[1][t]) + s_E[2][t]) + s_E[3][t];
  }
}

// Workgroup d adds the G <= MON_FT partials of dictionary index d as k_monitor_final does and writes its tag's entry; workgroup 0
// also writes the zeros of the entries that are no cell tag of the mesh.
__global__ __launch_bounds__(MON_FT) void k_stored_heat_final(int G, int tab_len, const double* __restrict__ part,
                                                             const uint8_t* __restrict__ slot_of_tag,
                                                             const int32_t* __restrict__ tag_of_slot, double* __restrict__ out) {
  __shared__ double s_E[16];
  const int d = blockIdx.x, t = threadIdx.x, wv = t >> 6, lane = t & 63;
  double a = t < G ? part[static_cast<size_t>(d) * G + t] : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma clang fp contract(off)
    a += __shfl_down(a, o, 64);
  }
  if (lane == 0) s_E[wv] = a;
  __syncthreads();
  if (t == 0) {
#pragma clang fp contract(off)
    for (int k = 1; k < MON_FT / 64; ++k) a += s_E[k];
    out[tag_of_slot[d]] = a;
  }
  if (d == 0)
    for (int k = t; k < tab_len; k += MON_FT)
      if (slot_of_tag[k] == MON_NONE) out[k] = 0.0;
}

void heat_free(hf_ctx* ctx) {
  hf_ctx::Heat& Q = ctx->heat;
  dev_free(&Q.slot); dev_free(&Q.tags); dev_free(&Q.none); dev_free(&Q.part); dev_free(&Q.now); dev_free(&Q.rec);
  Q = hf_ctx::Heat();
}

// The cumulative trapezoids of the capacity tables, on their first use (hf_set_capacity_form, hf_stored_heat)
int kt_ensure_cum(hf_ctx* ctx) {
  hf_ctx::KappaT& K = ctx->kt;
  if (!K.c_on || K.ccum) return HF_OK;
  std::vector<double> cum(K.h_cvals.size(), 0.0);
  for (const KTab& h : K.h_chdr)
    for (int i = 1; i < h.n; ++i) cum[h.off + i] = cum[h.off + i - 1] + 0.5 * (K.h_cvals[h.off + i - 1] + K.h_cvals[h.off + i]);
  HF_TRY(dev_alloc(ctx, &K.ccum, cum.size()));
  HF_HIP(copy_sync(ctx, K.ccum, cum.data(), sizeof(double) * cum.size(), hipMemcpyHostToDevice));
  return HF_OK;
}

// The buffers of the stored heat, on its first use: the dictionary is the row-gather tag dictionary, the schedule k_monitor's
int heat_ensure(hf_ctx* ctx) {
  hf_ctx::Heat& Q = ctx->heat;
  HF_TRY(kt_ensure_cum(ctx));
  if (Q.ready) return HF_OK;
  const int nd = static_cast<int>(std::min<size_t>(ctx->h_rg_tags.size(), MON_ND));
  std::vector<uint8_t> slot(static_cast<size_t>(ctx->tab_len), static_cast<uint8_t>(MON_NONE));
  std::vector<int32_t> tag_of(MON_ND, 0);
  for (int d = 0; d < nd; ++d) {
    const int32_t tg = ctx->h_rg_tags[d];
    if (tg >= 0 && tg < ctx->tab_len) slot[tg] = static_cast<uint8_t>(d);
    tag_of[d] = tg;
  }
  Q.nd = nd;
  Q.nchunks = (ctx->ne + MON_T - 1) / MON_T;
  Q.grid = std::min(Q.nchunks, MAXP);
  if (Q.grid >= 64) Q.grid &= ~7;
  const std::vector<KTab> none(MON_ND, KTab{0.0, 0.0, 0, 0});
  HF_TRY(dev_alloc(ctx, &Q.slot, static_cast<size_t>(ctx->tab_len)));
  HF_TRY(dev_alloc(ctx, &Q.tags, MON_ND));
  HF_TRY(dev_alloc(ctx, &Q.none, MON_ND));
  HF_TRY(dev_alloc(ctx, &Q.part, static_cast<size_t>(Q.grid) * MON_ND));
  HF_TRY(dev_alloc(ctx, &Q.now, static_cast<size_t>(ctx->tab_len)));
  HF_HIP(copy_sync(ctx, Q.slot, slot.data(), slot.size(), hipMemcpyHostToDevice));
  HF_HIP(copy_sync(ctx, Q.tags, tag_of.data(), sizeof(int32_t) * MON_ND, hipMemcpyHostToDevice));
  HF_HIP(copy_sync(ctx, Q.none, none.data(), sizeof(KTab) * MON_ND, hipMemcpyHostToDevice));
  Q.ready = true;
  return HF_OK;
}

// Room for n_more heat records behind the ones kept (as monitor_room: before the caller's first launch)
int heat_room(hf_ctx* ctx, int64_t n_more) {
  hf_ctx::Heat& Q = ctx->heat;
  if (!Q.rec_on) return HF_OK;
  HF_TRY(heat_ensure(ctx));      // (tables set after the switch: their cumulative trapezoids)
  if (Q.count + n_more <= Q.cap) return HF_OK;
  const int64_t cap = std::max<int64_t>(Q.count + n_more, 2 * Q.cap);
  double* grown = nullptr;
  HF_TRY(dev_alloc(ctx, &grown, static_cast<size_t>(cap) * ctx->tab_len));
  if (Q.count > 0) {
    const hipError_t e = copy_sync(ctx, grown, Q.rec, sizeof(double) * static_cast<size_t>(Q.count) * ctx->tab_len, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) { dev_free(&grown); return fail(ctx, HF_ERR_HIP, "heat records: copy failed: %s", hipGetErrorString(e)); }
  }
  dev_free(&Q.rec);
  Q.rec = grown;
  Q.cap = cap;
  return HF_OK;
}

// The two launches of one evaluation of the current state, on the stream, into `out` (tab_len doubles on the device)
void heat_launch(hf_ctx* ctx, double T_ref, double* out) {
  hf_ctx::Heat& Q = ctx->heat;
  const bool tabled = ctx->kt.c_on;
  hipLaunchKernelGGL(k_stored_heat, dim3(Q.grid), dim3(MON_T), static_cast<size_t>((ctx->tab_len + 15) & ~15), ctx->stream, ctx->ne,
                     Q.nchunks, ctx->tab_len, Q.nd, ctx->d_elem, ctx->d_zr, ctx->d_u, Q.slot, tabled ? ctx->kt.chdr : Q.none,
                     tabled ? ctx->kt.cvals : nullptr, tabled ? ctx->kt.ccum : nullptr, ctx->d_rhoc_rg, T_ref, Q.part);
  hipLaunchKernelGGL(k_stored_heat_final, dim3(Q.nd), dim3(MON_FT), 0, ctx->stream, Q.grid, ctx->tab_len, Q.part, Q.slot, Q.tags, out);
}

// The heat record of the step that has just been queued (the caller made room with heat_room)
inline void heat_record(hf_ctx* ctx) {
  hf_ctx::Heat& Q = ctx->heat;
  heat_launch(ctx, Q.T_ref, Q.rec + static_cast<size_t>(Q.count) * ctx->tab_len);
  Q.count += 1;
}

}  // namespace
