// Part of libheatflow_hip.so (see heatflow_hip.hip): device code - element assembly, CSR SpMV (LDS-staged and sub-wave), PCG and multigrid kernels
#pragma once
#include <type_traits>

#include "hf_context.hpp"

namespace {

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------

// Sum over the 256 threads of a workgroup, identical order every run: 64-lane shuffle tree
// per wavefront, then the four wave sums added in wave order.  Every thread gets the sum.
template <int NW = 4>
__device__ __forceinline__ double block_sum(double v, double* sw) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sw[w] = v;
  __syncthreads();
  double t = sw[0];
#pragma unroll
  for (int k = 1; k < NW; ++k) t += sw[k];
  __syncthreads();
  return t;
}

// Fixed-order sum of the P per-workgroup partials written by the previous kernel.
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int P, double* s4) {
  double v = 0.0;
  for (int k = threadIdx.x; k < P; k += TPB) v += part[k];
  return block_sum(v, s4);
}

// Chunk schedule of the row-chunked kernels.  Workgroups are dealt round-robin over the 8 XCDs
// (blockIdx % 8 says which blocks share an XCD and its L2; speed only, never correctness), so with
// HF_XCD_MAP each XCD group walks one contiguous eighth of the chunk range: spatially adjacent chunks
// (Morton order) then share an L2, which keeps the SpMV's neighbour gathers and a chunk's vector
// slices from kernel to kernel on the same XCD.  Every kernel uses the same schedule.
#ifndef HF_XCD_MAP
#define HF_XCD_MAP 1
#endif
struct ChunkIter {
  int chunk, step, end;
  __device__ __forceinline__ ChunkIter(int nchunks) {
    if (HF_XCD_MAP && (gridDim.x & 7) == 0) {
      const int per = (nchunks + 7) >> 3;
      const int xcd = blockIdx.x & 7;
      chunk = xcd * per + (blockIdx.x >> 3);
      step = gridDim.x >> 3;
      end = min(nchunks, (xcd + 1) * per);
    } else {
      chunk = blockIdx.x;
      step = gridDim.x;
      end = nchunks;
    }
  }
};

// r-weighted P1 element matrices (reference forms run_with_diamond.py:328-331).
//   M_ii = rho_c |K| (3 r_i + r_j + r_k)/30,  M_ij = rho_c |K| (2 r_i + 2 r_j + r_k)/60
//   K_ij = kappa |K| rbar (b_i b_j + c_i c_j)/d^2, d = 2*signed area, rbar = mean r
// m[] / k[] hold the symmetric 3x3 as {00, 11, 22, 01, 02, 12}.
__device__ __forceinline__ void element_local(const double2 p0, const double2 p1, const double2 p2, double rho_c,
                                              double kappa, double m[6], double k[6]) {
  // No FMA contraction here: the same element is evaluated by different workgroups (and by
  // different unrolled copies of the caller); every evaluation must give the same bits so that the
  // assembled matrices stay exactly symmetric.
#pragma clang fp contract(off)
  const double d = (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
  const double area = 0.5 * fabs(d);
  const double b0 = p1.y - p2.y, b1 = p2.y - p0.y, b2 = p0.y - p1.y;
  const double c0 = p2.x - p1.x, c1 = p0.x - p2.x, c2 = p1.x - p0.x;
  const double rsum = (p0.y + p1.y) + p2.y;
  const double ks = kappa * area * (rsum / 3.0) / (d * d);
  k[0] = ks * (b0 * b0 + c0 * c0);
  k[1] = ks * (b1 * b1 + c1 * c1);
  k[2] = ks * (b2 * b2 + c2 * c2);
  k[3] = ks * (b0 * b1 + c0 * c1);
  k[4] = ks * (b0 * b2 + c0 * c2);
  k[5] = ks * (b1 * b2 + c1 * c2);
  const double ms = rho_c * area;
  m[0] = ms * ((2.0 * p0.y + rsum) / 30.0);
  m[1] = ms * ((2.0 * p1.y + rsum) / 30.0);
  m[2] = ms * ((2.0 * p2.y + rsum) / 30.0);
  m[3] = ms * ((rsum + p0.y + p1.y) / 60.0);
  m[4] = ms * ((rsum + p0.y + p2.y) / 60.0);
  m[5] = ms * ((rsum + p1.y + p2.y) / 60.0);
}

__device__ __forceinline__ int sym_index(int a, int b) {  // (a,b) -> slot in {00,11,22,01,02,12}
  return a == b ? a : (a + b + 2);                        // 01->3, 02->4, 12->5
}

// ------------------------------------------------------------------------------------------
// Assembly, LDS-staged owner-computes.  Workgroup `blk` owns rows [blk*RBA, blk*RBA+RBA): it
// stages that slab of M and A (values) plus its column indices in LDS, walks the elements
// incident to its rows (precomputed list; an element on a block boundary is visited by each
// owning block, which adds only the rows it owns), and writes the slab out coalesced.
//   COLORED = false: LDS f64 atomics (ds_add_f64), any order
//   COLORED = true : elements grouped by colour (no two share an owned row), plain RMW,
//                    barrier between colours -> bitwise reproducible
// ------------------------------------------------------------------------------------------
// One list entry = 24 bytes = three int2: (n0, n1) (n2, tag<<11 | owned<<8 | off8) (off0..3, off4..7):
// the element record and the offsets of its nine contributions (a,b) = (0,0) (0,1) ... (2,2) inside
// the CSR rows of its nodes; `owned` marks the nodes whose rows this workgroup owns.
struct AsmEntry { int n0, n1, n2; unsigned w3, off03, off47; };

__device__ __forceinline__ AsmEntry load_entry(const int2* __restrict__ ent, int q) {
  const int2 a = ent[3 * q], b = ent[3 * q + 1], c = ent[3 * q + 2];
  return AsmEntry{a.x, a.y, b.x, static_cast<unsigned>(b.y), static_cast<unsigned>(c.x), static_cast<unsigned>(c.y)};
}

template <bool COLORED>
__global__ __launch_bounds__(RBA) void k_assemble_lds(int n, int cap, const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ blk_eptr,
                                                      const int32_t* __restrict__ blk_cptr,
                                                      const int2* __restrict__ blk_ent,
                                                      const double2* __restrict__ zr,
                                                      const double* __restrict__ kappa_tab,
                                                      const double* __restrict__ rhoc_tab, double dt,
                                                      double* __restrict__ Mv, double* __restrict__ Av) {
  extern __shared__ double smem[];
  // slab layout: the coloured variant keeps (M, A) of a slot side by side (one 16-byte read-modify-write per entry:
  // 80 -> 74 us at C3); the atomic variant keeps two arrays (atomics on neighbouring words collide: 50 vs 56 us)
  double2* sMA = reinterpret_cast<double2*>(smem);
  double* sM = smem;
  double* sA = smem + cap;
  int* sR = reinterpret_cast<int*>(smem + 2 * cap);

  const int blk = blockIdx.x;
  const int r0 = blk * RBA;
  const int r1 = min(n, r0 + RBA);
  const int k0 = rowptr[r0];
  const int nk = rowptr[r1] - k0;
  for (int k = threadIdx.x; k < nk; k += RBA) {
    if (COLORED) {
      sMA[k] = make_double2(0.0, 0.0);
    } else {
      sM[k] = 0.0;
      sA[k] = 0.0;
    }
  }
  for (int k = threadIdx.x; k <= r1 - r0; k += RBA) sR[k] = rowptr[r0 + k] - k0;
  __syncthreads();

  auto scatter = [&](const AsmEntry e, const double2 p0, const double2 p1, const double2 p2) {
    double m[6], kk[6], av6[6];
    const int tag = static_cast<int>(e.w3 >> 11);
    element_local(p0, p1, p2, rhoc_tab[tag], kappa_tab[tag], m, kk);
#pragma unroll
    for (int q = 0; q < 6; ++q) av6[q] = fma(dt, kk[q], m[q]);  // once per unique entry, explicit FMA: same bits everywhere
    const int nd[3] = {e.n0, e.n1, e.n2};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!((e.w3 >> (8 + a)) & 1u)) continue;
      const int base = sR[nd[a] - r0];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const int q9 = a * 3 + b;
        const unsigned off = q9 < 4 ? (e.off03 >> (8 * q9)) & 0xFFu : q9 < 8 ? (e.off47 >> (8 * (q9 - 4))) & 0xFFu : e.w3 & 0xFFu;
        const int slot = base + static_cast<int>(off);
        const int q = sym_index(a, b);
        if (COLORED) {
          double2 t = sMA[slot];
          t.x += m[q];
          t.y += av6[q];
          sMA[slot] = t;
        } else {
          atomicAdd(&sM[slot], m[q]);
          atomicAdd(&sA[slot], av6[q]);
        }
      }
    }
  };
  // The list is laid out per workgroup and streamed coalesced; only the coordinates are gathered.
  // Three elements in flight per lane: all loads are issued before the first scatter.
  constexpr int NF = 3;
  auto run_range = [&](int e0, int e1) {
    for (int k = e0 + threadIdx.x; k < e1; k += NF * RBA) {
      AsmEntry e[NF];
      double2 pa[NF], pb[NF], pc[NF];
#pragma unroll
      for (int u = 0; u < NF; ++u) e[u] = load_entry(blk_ent, min(k + u * RBA, e1 - 1));
#pragma unroll
      for (int u = 0; u < NF; ++u) { pa[u] = zr[e[u].n0]; pb[u] = zr[e[u].n1]; pc[u] = zr[e[u].n2]; }
#pragma unroll
      for (int u = 0; u < NF; ++u)
        if (k + u * RBA < e1) scatter(e[u], pa[u], pb[u], pc[u]);
    }
  };

  if (COLORED) {
    const int32_t* cp = blk_cptr + static_cast<size_t>(blk) * (NCOL + 1);
    for (int c = 0; c < NCOL; ++c) {
      const int e0 = cp[c], e1 = cp[c + 1];
      if (e0 == e1) { if (e1 == cp[NCOL]) break; else continue; }
      run_range(e0, e1);
      __syncthreads();
    }
  } else {
    run_range(blk_eptr[blk], blk_eptr[blk + 1]);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nk; k += RBA) {
    if (COLORED) {
      const double2 t = sMA[k];
      Mv[k0 + k] = t.x;
      Av[k0 + k] = t.y;
    } else {
      Mv[k0 + k] = sM[k];
      Av[k0 + k] = sA[k];
    }
  }
}

// ------------------------------------------------------------------------------------------
// Assembly, row gather (HF_ASM_ROW_GATHER): the element routines, then one body (rowgather_assemble) behind the five kernels
// k_assemble_rows, k_assemble_rows_an, k_assemble_rows_kT, k_assemble_rows_cT and k_assemble_rows_kT_K, and the table kernels'
// three siblings on anisotropic tags (k_assemble_rows_kT_an, k_assemble_rows_cT_an, k_assemble_rows_kT_K_an).
// Every triangle is evaluated once per vertex ("me", next, previous in the triangle's own cyclic
// order).  The formulas are symmetric by construction, so the three evaluations agree bit for bit
// where they must (A_ij == A_ji) without agreeing on a vertex order:
//   edges   e_v = P_next(v) - P_prev(v): the same subtraction from every vertex's point of view
//   K_ab  = ks * (e_a . e_b)             (products commute)
//   d     = max |e_a x e_b| over the three edge pairs (three roundings of twice the area)
//   rsum  = (lo + mid) + hi of the three radii sorted by value
//   M_aa  = ms/30 * (2 r_a + rsum),  M_ab = ms/60 * (rsum + (r_a + r_b))
// One IEEE division per evaluation (1/d^2); constant divisors are multiplications by rounded reciprocals.
// ------------------------------------------------------------------------------------------
struct ElemRow { double m0, m1, m2, k0, k1, k2; };   // row "me" of the element matrices: (me,me) (me,next) (me,prev)

// (lo + mid) + hi of three values sorted by value: the same bits in whichever order they are given (rsum, and 3 T_e of the tables)
__device__ __forceinline__ double sorted_sum3(double a, double b, double c) {
#pragma clang fp contract(off)
  const double ab_lo = fmin(a, b), ab_hi = fmax(a, b);
  const double lo = fmin(ab_lo, c), hi = fmax(ab_hi, c), mid = fmax(ab_lo, fmin(ab_hi, c));
  return (lo + mid) + hi;
}

// Anisotropic element stiffness (hf_set_anisotropy): the tensor diag(k_z, k_r) in (z, r), constant per element.  The gradient of
// a hat function is perpendicular to the opposite edge, so the z-differences of the edges carry k_r and the r-differences k_z:
//   K_ab = ks * (k_r * (e_a.x * e_b.x) + k_z * (e_a.y * e_b.y)),  ks = area * (rsum / 3) / d^2
// Everything else - edges, d, rsum, M - is the isotropic row's, and the products commute, so the three per-vertex evaluations of
// a triangle still agree bit for bit (A stays exactly symmetric).
// ANISO = false: K_ab = ks * (e_a . e_b), ks = k_z * area * (rsum / 3) / d^2 (k_z holds kappa, k_r is not used).
// One routine with both formulas statement for statement, not a geometry helper under two callers: the helper (tried with a
// functor for the stiffness form) made the compiler commute k_assemble_rows_an's v_add_f64 operands.  The bits stay either way,
// the machine code does not; keep the order of the statements.
template <bool ANISO>
__device__ __forceinline__ ElemRow element_row_of(const double2 Pi, const double2 Pj, const double2 Pk, double rho_c, double k_z, double k_r) {
#pragma clang fp contract(off)
  const double eix = Pk.x - Pj.x, eiy = Pk.y - Pj.y;     // edge opposite "me"
  const double ejx = Pi.x - Pk.x, ejy = Pi.y - Pk.y;     // opposite next
  const double ekx = Pj.x - Pi.x, eky = Pj.y - Pi.y;     // opposite previous
  const double c1 = fabs(ejx * eky - ejy * ekx), c2 = fabs(ekx * eiy - eky * eix), c3 = fabs(eix * ejy - eiy * ejx);
  const double d = fmax(fmax(c1, c2), c3);
  const double rsum = sorted_sum3(Pi.y, Pj.y, Pk.y);
  const double area = 0.5 * d;
  const double ks = ANISO ? area * (rsum * (1.0 / 3.0)) * (1.0 / (d * d)) : k_z * area * (rsum * (1.0 / 3.0)) * (1.0 / (d * d));
  const double ms30 = rho_c * area * (1.0 / 30.0), ms60 = rho_c * area * (1.0 / 60.0);
  ElemRow o;
  o.k0 = ks * (ANISO ? k_r * (eix * eix) + k_z * (eiy * eiy) : eix * eix + eiy * eiy);
  o.k1 = ks * (ANISO ? k_r * (eix * ejx) + k_z * (eiy * ejy) : eix * ejx + eiy * ejy);
  o.k2 = ks * (ANISO ? k_r * (eix * ekx) + k_z * (eiy * eky) : eix * ekx + eiy * eky);
  o.m0 = ms30 * (2.0 * Pi.y + rsum);
  o.m1 = ms60 * (rsum + (Pi.y + Pj.y));
  o.m2 = ms60 * (rsum + (Pi.y + Pk.y));
  return o;
}

__device__ __forceinline__ ElemRow element_row(const double2 Pi, const double2 Pj, const double2 Pk, double rho_c, double kappa) {
  return element_row_of<false>(Pi, Pj, Pk, rho_c, kappa, 0.0);
}

__device__ __forceinline__ ElemRow element_row_an(const double2 Pi, const double2 Pj, const double2 Pk, double rho_c, double k_z, double k_r) {
  return element_row_of<true>(Pi, Pj, Pk, rho_c, k_z, k_r);
}

// V::STATE2 (optional member, STATE only): a second state is staged behind the first (sU2; v.state2(node)), and a visit receives both
template <class V, class = void>
struct rg_state2 : std::false_type {};
template <class V>
struct rg_state2<V, std::void_t<decltype(V::STATE2)>> : std::bool_constant<V::STATE2> {};

constexpr int RG_NC = 4;   // 16-byte vectors of column positions a lane can prefetch (RBA * 8 * RG_NC >= slab slots: rows hold <= 32 entries)
constexpr int RG_NX = 5;   // coordinate pairs a lane can prefetch (RBA * RG_NX >= column-list length, checked on the host)

// The body of the row-gather kernels.  Lane t of a workgroup owns CSR row r0 + t and visits the
// triangles at its node one after another (ELL slab of 16-bit entries, hf_pattern.hpp RowGather).  A
// triangle is described by the positions of its two other vertices inside the row's column list, so a
// contribution's slot is known without any search or offset table, and the element array is never read.
// Per block of RBA rows the kernel stages, all as coalesced 16-byte streams: the rows' 16-bit column
// positions, the coordinates of the block's column list (own rows + halo, a per-block copy made at
// hf_set_mesh) and its ELL entries; the value slab lives in LDS and is streamed out once.  The
// visit loop touches LDS only.  Rows are private to their lane: no atomics, no colours, no barriers
// inside the loop, and the order of additions is the list order - bitwise reproducible.
// Workgroups are persistent: while block b is computed the loads of the workgroup's next block are in
// flight into registers and the stores of its previous block drain, so the three phases overlap.
// What a kernel adds is its coefficient policy V:
//   V::PAIR    the slab holds (M, A) as a double2 per slot, else one double
//   V::STATE   the block's slice of an evaluation state is staged next to the coordinates (sU; dict: the column lists' node ids)
//   V::KONLY   the stiffness alone: no M half, no dt
//   V::NODE_FIRST  (STATE only) the prefetch reads the node id in a guarded load of its own before the state, as the kernels
//              with a two-array state were written, or inside the state's guard.  The same values either way, but the compiler
//              schedules the two spellings differently, and each kernel keeps the machine code it had
//              (profiles/rowgather_unify_asm_compare.txt)
//   V::ID      its RgVariant: the host's index of the kernel's cached grid
//   v.state(node)                              the evaluation state at a node (STATE only)
//   v.row(tg, Pi, Pj, Pk, sU, ui, cj, ck)      the ElemRow of a visit: tg the tag-dictionary index, cj / ck the other two
//                                              vertices' positions in the column list, ui = sU[my own position]
//   v.dt                                       of A = M + dt K (not KONLY)
// Out: PAIR - Mv (not KONLY) and Av; one value - Av alone.
template <class V>
__device__ __forceinline__ void rowgather_assemble(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                   const int32_t* __restrict__ rowptr, const int4* __restrict__ hdr /* 2 per block */,
                                                   const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                   const double2* __restrict__ zrb, const int32_t* __restrict__ dict, const V v,
                                                   double* __restrict__ Mv, double* __restrict__ Av, double* smem) {
  using Slot = std::conditional_t<V::PAIR, double2, double>;
  constexpr bool S2 = rg_state2<V>::value;
  if constexpr (S2) static_assert(V::STATE && V::NODE_FIRST, "the second state is prefetched next to the first, in the NODE_FIRST spelling");
  Slot* sS = reinterpret_cast<Slot*>(smem);                          // (M, A), A or K per slot
  double2* sXd = reinterpret_cast<double2*>(sS + cap);               // coordinates of the block's column list
  double* sU = reinterpret_cast<double*>(sXd + capd);                // STATE: the evaluation state on the block's column list
  double* sU2 = sU + capd + (capd & 1);                              // STATE2: the second state behind it
  int* sR = reinterpret_cast<int*>(S2 ? sU2 + capd + (capd & 1) : V::STATE ? sU + capd + (capd & 1) : sU);   // row starts inside the slab
  uint4* sC4 = reinterpret_cast<uint4*>(sR + RBA + 4);               // column-list position per slot, from the 8-aligned start
  const uint16_t* sC = reinterpret_cast<const uint16_t*>(sC4);

  const int t = threadIdx.x;
  for (int k = t; k < cap; k += RBA) sS[k] = Slot();

  // prefetch registers of the next block
  int4 hA, hB;
  uint4 pe, pc[RG_NC];
  double2 px[RG_NX];
  double pu[V::STATE ? RG_NX : 1];
  double pu2[S2 ? RG_NX : 1];
  int pr = 0;
  auto prefetch = [&](int blk) {
    hA = hdr[2 * blk];                                               // (k0, nk, d0, nd)
    hB = hdr[2 * blk + 1];                                           // (ell offset in 16-byte units, groups of 8 visits, local id of row r0, rows)
    pe = ell[hB.x + t];
    const int c0 = hA.x >> 3, nc = ((hA.x + hA.y + 7) >> 3) - c0;
#pragma unroll
    for (int q = 0; q < RG_NC; ++q) pc[q] = (t + q * RBA < nc) ? cid16[c0 + t + q * RBA] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < RG_NX; ++q) {
      const bool in = t + q * RBA < hA.w;
      px[q] = in ? zrb[hA.z + t + q * RBA] : make_double2(0.0, 0.0);
      if constexpr (V::STATE) {
        if constexpr (V::NODE_FIRST) {
          const int node = in ? dict[hA.z + t + q * RBA] : 0;
          pu[q] = in ? v.state(node) : 0.0;
          if constexpr (S2) pu2[q] = in ? v.state2(node) : 0.0;
        } else {
          pu[q] = in ? v.state(dict[hA.z + t + q * RBA]) : 0.0;
        }
      }
    }
    pr = (t < hB.w) ? rowptr[blk * RBA + t] - hA.x : 0;
  };
  int blk = blockIdx.x;
  if (blk < nblk) prefetch(blk);
  while (blk < nblk) {
    // stage the prefetched block
    const int4 cA = hA, cB = hB;
    const uint4 ce = pe;
    const int nc = ((cA.x + cA.y + 7) >> 3) - (cA.x >> 3);
#pragma unroll
    for (int q = 0; q < RG_NC; ++q) if (t + q * RBA < nc) sC4[t + q * RBA] = pc[q];
#pragma unroll
    for (int q = 0; q < RG_NX; ++q)
      if (t + q * RBA < cA.w) {
        sXd[t + q * RBA] = px[q];
        if constexpr (V::STATE) sU[t + q * RBA] = pu[q];
        if constexpr (S2) sU2[t + q * RBA] = pu2[q];
      }
    sR[t] = pr;
    __syncthreads();
    const int nxt = blk + gridDim.x;
    if (nxt < nblk) prefetch(nxt);                                   // in flight during the visit loop

    if (t < cB.w) {
      const int base = sR[t];
      const int sbase = base + (cA.x & 7);                           // the position array starts at the 8-aligned slot
      const int ci = cB.z + t;                                       // my own position in the column list
      const double2 Pi = sXd[ci];
      double ui = 0.0;
      if constexpr (V::STATE) ui = sU[ci];
      double ui2 = 0.0;
      if constexpr (S2) ui2 = sU2[ci];
      double dM = 0.0, dA = 0.0;
      int pd = 0;                                                    // diagonal: the slot whose column is my own row
      while (pd < 31 && sC[sbase + pd] < ci) ++pd;
      for (int g = 0; g < cB.y; ++g) {
        const uint4 ev = g == 0 ? ce : ell[cB.x + g * RBA + t];
        const unsigned w[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const unsigned e = (w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
          if (e == 0xFFFFu) continue;
          const int pj = e & 31u, pk = (e >> 5) & 31u, tg = e >> 10;
          const int cj = sC[sbase + pj], ck = sC[sbase + pk];
          const double2 Pj = sXd[cj], Pk = sXd[ck];
          ElemRow r;
          if constexpr (S2) r = v.row(tg, Pi, Pj, Pk, sU, ui, sU2, ui2, cj, ck);
          else r = v.row(tg, Pi, Pj, Pk, sU, ui, cj, ck);
          if constexpr (V::PAIR && V::KONLY) {
            dA += r.k0;
            sS[base + pj].y += r.k1;
            sS[base + pk].y += r.k2;
          } else if constexpr (V::PAIR) {
            dM += r.m0;
            dA += fma(v.dt, r.k0, r.m0);
            double2 s = sS[base + pj];
            s.x += r.m1;
            s.y += fma(v.dt, r.k1, r.m1);
            sS[base + pj] = s;
            s = sS[base + pk];
            s.x += r.m2;
            s.y += fma(v.dt, r.k2, r.m2);
            sS[base + pk] = s;
          } else if constexpr (V::KONLY) {
            dA += r.k0;
            sS[base + pj] += r.k1;
            sS[base + pk] += r.k2;
          } else {
            dA += fma(v.dt, r.k0, r.m0);
            sS[base + pj] += fma(v.dt, r.k1, r.m1);
            sS[base + pk] += fma(v.dt, r.k2, r.m2);
          }
        }
      }
      if constexpr (V::PAIR) sS[base + pd] = make_double2(dM, dA);
      else sS[base + pd] = dA;
    }
    __syncthreads();
    // stream the slab out and leave it zeroed for the next block (slot k stays with the lane that reads it here)
    for (int k = t; k < cA.y; k += RBA) {
      const Slot s = sS[k];
      if constexpr (V::PAIR) {
        if (!V::KONLY) Mv[cA.x + k] = s.x;
        Av[cA.x + k] = s.y;
      } else {
        Av[cA.x + k] = s;
      }
      sS[k] = Slot();
    }
    blk = nxt;
    // no barrier needed here: the staging stores above touch sC / sXd / sU / sR only after every lane has passed the
    // barrier that ended the visit loop, and the slab is re-read only behind the next staging barrier
  }
}

// (m_z, m_r) of a tag on top of its kappa: k_z = m_z kappa along z, k_r = m_r kappa along r.  m_z == m_r goes through element_row
// with kappa * m (x * 1.0 is exact: multipliers 1 give the isotropic bits), anything else through element_row_an.
__device__ __forceinline__ ElemRow element_row_m(const double2 Pi, const double2 Pj, const double2 Pk, double rho_c, double kappa, const double2 m) {
  return m.x == m.y ? element_row(Pi, Pj, Pk, rho_c, kappa * m.x) : element_row_an(Pi, Pj, Pk, rho_c, m.x * kappa, m.y * kappa);
}

// Constant coefficients by tag-dictionary index.  K (the steady operator, hf_steady_setup): Av receives K, the slab's M half
// stays zero, Mv is not written (may be null); rhoc_idx and dt are not used.
// AN (hf_set_anisotropy, k_assemble_rows_an): a second 64-entry table by tag-dictionary index, an_idx[tg] = (m_z, m_r), through
// element_row_m.  With every multiplier 1 M and A come out bit for bit as k_assemble_rows gives them, and in a mixed mesh every
// row that touches only elements of tags with m_z == m_r keeps its bits.  Not AN: an_idx is not used.
template <bool K, bool AN>
struct RowsConst {
  static constexpr bool PAIR = true, STATE = false, KONLY = K;
  static constexpr RgVariant ID = AN ? (K ? RG_AN_K : RG_AN) : (K ? RG_ROWS_K : RG_ROWS);
  const double *kappa_idx, *rhoc_idx;
  const double2* an_idx;
  double dt;
  __device__ __forceinline__ ElemRow row(int tg, const double2 Pi, const double2 Pj, const double2 Pk, const double*, double, int, int) const {
    const double2 m = AN ? an_idx[tg] : make_double2(1.0, 1.0);   // read first: with kappa_idx first k_assemble_rows_an compiles otherwise
    const double kappa = kappa_idx[tg], rho_c = K ? 0.0 : rhoc_idx[tg];
    if constexpr (AN) return element_row_m(Pi, Pj, Pk, rho_c, kappa, m);
    else return element_row(Pi, Pj, Pk, rho_c, kappa);
  }
};

template <bool KONLY>
__global__ __launch_bounds__(RBA) void k_assemble_rows(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                       const int32_t* __restrict__ rowptr,
                                                       const int4* __restrict__ hdr /* 2 per block */,
                                                       const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                       const double2* __restrict__ zrb,
                                                       const double* __restrict__ kappa_idx, const double* __restrict__ rhoc_idx,
                                                       double dt, double* __restrict__ Mv, double* __restrict__ Av) {
  extern __shared__ double smem[];
  rowgather_assemble(nblk, cap, capd, rowptr, hdr, ell, cid16, zrb, nullptr, RowsConst<KONLY, false>{kappa_idx, rhoc_idx, nullptr, dt}, Mv, Av, smem);
}

template <bool KONLY>
__global__ __launch_bounds__(RBA) void k_assemble_rows_an(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                          const int32_t* __restrict__ rowptr,
                                                          const int4* __restrict__ hdr /* 2 per block */,
                                                          const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                          const double2* __restrict__ zrb,
                                                          const double* __restrict__ kappa_idx, const double* __restrict__ rhoc_idx,
                                                          const double2* __restrict__ an_idx /* (m_z, m_r) */,
                                                          double dt, double* __restrict__ Mv, double* __restrict__ Av) {
  extern __shared__ double smem[];
  rowgather_assemble(nblk, cap, capd, rowptr, hdr, ell, cid16, zrb, nullptr, RowsConst<KONLY, true>{kappa_idx, rhoc_idx, an_idx, dt}, Mv, Av, smem);
}

// What a load policy sees of the block's LDS: the column list's coordinates, its own per-node doubles behind them (sN; arrays
// of capw = capd + (capd & 1) doubles first, then any interleaved columns), the rows' 16-bit column positions and capd.
struct VisitLds {
  double2* sXd;
  double* sN;
  const uint16_t* sC;
  int capd;
  __device__ __forceinline__ int capw() const { return capd + (capd & 1); }
};

// The body of the row-visit load kernels: rowgather_assemble's lists and block staging (without its register prefetch), but a
// visit adds to registers of the row's lane, not to a slab - lane t of a workgroup owns row blk * RBA + t, walks the triangles at
// its node in list order and stores once.  No atomics, no LDS accumulation: bitwise reproducible.  Per block of RBA rows the
// body stages the rows' 16-bit column positions, the coordinates of the block's column list and the row starts; the visit loop
// touches LDS only.  What a kernel adds is its load policy V:
//   V::NODE, V::WIDE     per-node doubles in LDS behind the coordinates: NODE arrays of capw doubles, then capd * WIDE
//                        interleaved ones (rounded up to even; 0: none).  rowvisit_lds_bytes (hf_pattern.hpp) sizes the launch
//                        from the same two numbers
//   V::OCC_GRID, V::ID   launch_rowvisit: a grid from one occupancy query cached in rg_grid[ID], else min(blocks, 2048)
//   v.tables(t)          lane t < 64 fills entry t of the policy's by-tag tables (static LDS of the kernel)
//   v.node(L, i, P, dict, g)   fill the per-node doubles of column slot i: P its coordinates, dict[g] its node id
//   v.begin(L, ci)       the row's state: its own values (ci = its position in the column list) and zeroed accumulators
//   row = v.visit(L, row, Pi, tg, ij, ik)   one triangle, row state in and out by value: tg the tag-dictionary index,
//                        L.sC[ij] / L.sC[ik] the other two vertices' positions in the column list; early-outs come before those reads
//   v.store(row, r)      write row r
// The visit loop runs without contraction; a policy's functions state `fp contract(off)` themselves where they do arithmetic.
template <class V>
__device__ __forceinline__ void rowgather_visit(int nblk, int capd, const int4* __restrict__ hdr, const uint4* __restrict__ ell,
                                                const uint4* __restrict__ cid16, const double2* __restrict__ zrb,
                                                const int32_t* __restrict__ dict, const int32_t* __restrict__ rowptr, const V v,
                                                double* smem) {
  double2* sXd = reinterpret_cast<double2*>(smem);
  double* sN = smem + 2 * capd;
  const int capw = capd + (capd & 1);
  static_assert(V::NODE >= 1 && V::NODE <= 3, "one to three per-node arrays");
  double* sEnd = sN + capw;                                          // array by array, as the kernels carved it up
  if constexpr (V::NODE > 1) sEnd += capw;
  if constexpr (V::NODE > 2) sEnd += capw;
  int* sR = reinterpret_cast<int*>(sEnd + ((capd * V::WIDE + 1) & ~1));    // row starts
  uint4* sC4 = reinterpret_cast<uint4*>(sR + RBA + 4);
  const uint16_t* sC = reinterpret_cast<const uint16_t*>(sC4);
  const VisitLds L{sXd, sN, sC, capd};
  const int t = threadIdx.x;
  if (t < 64) v.tables(t);
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int4 cA = hdr[2 * blk], cB = hdr[2 * blk + 1];
    const int c0 = cA.x >> 3, nc = ((cA.x + cA.y + 7) >> 3) - c0;
    for (int i = t; i < nc; i += RBA) sC4[i] = cid16[c0 + i];
    for (int i = t; i < cA.w; i += RBA) {
      const double2 P = zrb[cA.z + i];
      sXd[i] = P;
      v.node(L, i, P, dict, cA.z + i);
    }
    if (t < cB.w) sR[t] = rowptr[blk * RBA + t] - cA.x;
    __syncthreads();
    if (t < cB.w) {
#pragma clang fp contract(off)
      const int sbase = sR[t] + (cA.x & 7);
      const int ci = cB.z + t;
      const double2 Pi = sXd[ci];
      auto row = v.begin(L, ci);
      for (int g = 0; g < cB.y; ++g) {
        const uint4 ev = ell[cB.x + g * RBA + t];
        const unsigned w[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const unsigned e = (w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
          if (e == 0xFFFFu) continue;
          row = v.visit(L, row, Pi, static_cast<int>(e >> 10), sbase + (e & 31u), sbase + ((e >> 5) & 31u));
        }
      }
      v.store(row, blk * RBA + t);
    }
    __syncthreads();
  }
}

// The load kernels that keep a body of their own (k_tangent_load, _dir, _cap, _T and k_source_load_d: folded into the body
// above they compile to other registers, see profiles/rowvisit_unify_asm_compare.txt) state only what launch_rowvisit reads
// of a policy: their per-node LDS and their grid rule.
template <int N, int W, bool OCC = false, RgVariant I = RG_VARIANTS>
struct VisitLaunch {
  static constexpr int NODE = N, WIDE = W;
  static constexpr bool OCC_GRID = OCC;
  static constexpr RgVariant ID = I;
};
using VisitLoad = VisitLaunch<1, 0>;                          // sU; also k_tangent_load_dir and, with sW for sU, k_tangent_load_cap
using VisitSourceD = VisitLaunch<2, 0, true, RG_SOURCE_D>;    // sF, sD
template <int NV>
using VisitTables = VisitLaunch<3, NV, true, NV == 2 ? RG_TLT2 : NV == 4 ? RG_TLT4 : NV == 8 ? RG_TLT8 : RG_TLT16>;   // sU, sW, sE, s*

// The step rate of a node from u = u^{n+1}, un = u^n and um1 = u^{n-1}: 0 (wmode 0, no step taken), (u - un) / dtp (1: backward
// Euler), ((u - 4/3 un) + 1/3 um1) / dtp (2: BDF2).  The one spelling for every kernel that stages w: a node's w has the same bits
// in all of them.  un and um1 are read only where the mode uses them.
__device__ __forceinline__ double step_rate(double u1, const double* __restrict__ un, const double* __restrict__ um1, int node,
                                            int wmode, double dtp) {
#pragma clang fp contract(off)
  double w = 0.0;
  if (wmode == 1) w = (u1 - un[node]) / dtp;
  else if (wmode == 2) w = ((u1 - (4.0 / 3.0) * un[node]) + (1.0 / 3.0) * um1[node]) / dtp;
  return w;
}

// Read-flux projection right-hand sides by row gather (same lists and staging as k_assemble_rows, plus the block's
// slice of the state u): b_c[i] = sum over the triangles at node i of (d_c T)_e * |K| (2 r_i + r_j + r_k)/12, summed
// in list order in a register - no LDS accumulation, no atomics, bitwise reproducible.
struct VisitGrad {
  static constexpr int NODE = 1, WIDE = 0;                 // sU: the state
  static constexpr bool OCC_GRID = false;
  const double* u;
  double *bz, *br;
  int stride, ustride, uoff;
  struct Row { double ui, az, ar; };
  __device__ __forceinline__ void tables(int) const {}
  __device__ __forceinline__ void node(const VisitLds& L, int i, double2, const int32_t* __restrict__ dict, int g) const {
    L.sN[i] = u[static_cast<size_t>(dict[g]) * ustride + uoff];
  }
  __device__ __forceinline__ Row begin(const VisitLds& L, int ci) const { return Row{L.sN[ci], 0.0, 0.0}; }
  __device__ __forceinline__ Row visit(const VisitLds& L, Row r, const double2 Pi, int, unsigned ij, unsigned ik) const {
#pragma clang fp contract(off)
    const double* sU = L.sN;
    const int cj = L.sC[ij], ck = L.sC[ik];
    const double2 Pj = L.sXd[cj], Pk = L.sXd[ck];
    const double ui = r.ui, uj = sU[cj], uk = sU[ck];
    const double d = (Pj.x - Pi.x) * (Pk.y - Pi.y) - (Pk.x - Pi.x) * (Pj.y - Pi.y);
    const double gz = (ui * (Pj.y - Pk.y) + uj * (Pk.y - Pi.y) + uk * (Pi.y - Pj.y)) / d;
    const double gr = (ui * (Pk.x - Pj.x) + uj * (Pi.x - Pk.x) + uk * (Pj.x - Pi.x)) / d;
    const double wgt = 0.5 * fabs(d) * (Pi.y + ((Pi.y + Pj.y) + Pk.y)) / 12.0;
    r.az += gz * wgt;
    r.ar += gr * wgt;
    return r;
  }
  __device__ __forceinline__ void store(const Row& r, int row) const {
    if (bz != nullptr) bz[static_cast<size_t>(row) * stride] = r.az;
    if (br != nullptr) br[static_cast<size_t>(row) * stride] = r.ar;
  }
};

__global__ __launch_bounds__(RBA) void k_grad_rows(int nblk, int capd, const int4* __restrict__ hdr, const uint4* __restrict__ ell,
                                                   const uint4* __restrict__ cid16, const double2* __restrict__ zrb,
                                                   const int32_t* __restrict__ dict, const int32_t* __restrict__ rowptr,
                                                   const double* __restrict__ u, double* __restrict__ bz, double* __restrict__ br,
                                                   int stride /* of the outputs - 1: plain arrays; 2: bz = out, br = out + 1 interleaved; nv: column j of an interleaved batch vector */,
                                                   int ustride, int uoff /* the state is u[node * ustride + uoff] (batched loop: column uoff of nv) */) {
  extern __shared__ double smem[];
  rowgather_visit(nblk, capd, hdr, ell, cid16, zrb, dict, rowptr, VisitGrad{u, bz, br, stride, ustride, uoff}, smem);
}

// Per-parameter stiffness products of a tangent run (hf_run_tangent) by row gather (same lists and staging as k_grad_rows):
// F[i * NV + j] = -sum over the triangles e at node i whose tag maps to column j (col[tag-dictionary index] = j) of
// (K_e u)_i, K_e the r-weighted element stiffness at unit conductivity (element_row, as k_assemble_rows<true> forms it).
// One pass over the triangles serves all NV columns: u is read once, K_j is never formed.  Each column's sum runs in list
// order in a register of the row's lane - bitwise reproducible; columns no tag maps to are written as zeros.
template <int NV>
__global__ __launch_bounds__(RBA) void k_tangent_load(int nblk, int capd, const int4* __restrict__ hdr, const uint4* __restrict__ ell,
                                                      const uint4* __restrict__ cid16, const double2* __restrict__ zrb,
                                                      const int32_t* __restrict__ dict, const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, const double* __restrict__ u,
                                                      double* __restrict__ F) {
  extern __shared__ double smem[];
  __shared__ int scol[64];
  double2* sXd = reinterpret_cast<double2*>(smem);
  double* sU = smem + 2 * capd;
  int* sR = reinterpret_cast<int*>(sU + capd + (capd & 1));
  uint4* sC4 = reinterpret_cast<uint4*>(sR + RBA + 4);
  const uint16_t* sC = reinterpret_cast<const uint16_t*>(sC4);
  const int t = threadIdx.x;
  if (t < 64) scol[t] = col[t];
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int4 cA = hdr[2 * blk], cB = hdr[2 * blk + 1];
    const int c0 = cA.x >> 3, nc = ((cA.x + cA.y + 7) >> 3) - c0;
    for (int i = t; i < nc; i += RBA) sC4[i] = cid16[c0 + i];
    for (int i = t; i < cA.w; i += RBA) { sXd[i] = zrb[cA.z + i]; sU[i] = u[dict[cA.z + i]]; }
    if (t < cB.w) sR[t] = rowptr[blk * RBA + t] - cA.x;
    __syncthreads();
    if (t < cB.w) {
#pragma clang fp contract(off)
      const int sbase = sR[t] + (cA.x & 7);
      const int ci = cB.z + t;
      const double2 Pi = sXd[ci];
      const double ui = sU[ci];
      double acc[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] = 0.0;
      for (int g = 0; g < cB.y; ++g) {
        const uint4 ev = ell[cB.x + g * RBA + t];
        const unsigned w[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const unsigned e = (w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
          if (e == 0xFFFFu) continue;
          const int cj = scol[e >> 10];
          if (cj < 0) continue;
          const int pj = sC[sbase + (e & 31u)], pk = sC[sbase + ((e >> 5) & 31u)];
          const ElemRow r = element_row(Pi, sXd[pj], sXd[pk], 0.0, 1.0);
          const double ku = (r.k0 * ui + r.k1 * sU[pj]) + r.k2 * sU[pk];
#pragma unroll
          for (int j = 0; j < NV; ++j)
            if (j == cj) acc[j] += ku;
        }
      }
      double* out = F + static_cast<size_t>(blk * RBA + t) * NV;
#pragma unroll
      for (int j = 0; j < NV; ++j) out[j] = -acc[j];
    }
    __syncthreads();
  }
}

// (K^r u)_me and (K^z u)_me of one element visit at unit conductivities, in the letters of element_row_of:
// K^r_ab = ks (e_a.x e_b.x), K^z_ab = ks (e_a.y e_b.y), ks = area (rsum / 3) / d^2 - one division, as there.
struct DirKu { double r, z; };
__device__ __forceinline__ DirKu element_dir_ku(const double2 Pi, const double2 Pj, const double2 Pk, double ui, double uj, double uk) {
#pragma clang fp contract(off)
  const double eix = Pk.x - Pj.x, eiy = Pk.y - Pj.y;     // edge opposite "me"
  const double ejx = Pi.x - Pk.x, ejy = Pi.y - Pk.y;     // opposite next
  const double ekx = Pj.x - Pi.x, eky = Pj.y - Pi.y;     // opposite previous
  const double c1 = fabs(ejx * eky - ejy * ekx), c2 = fabs(ekx * eiy - eky * eix), c3 = fabs(eix * ejy - eiy * ejx);
  const double d = fmax(fmax(c1, c2), c3);
  const double rsum = sorted_sum3(Pi.y, Pj.y, Pk.y);
  const double area = 0.5 * d;
  const double ks = area * (rsum * (1.0 / 3.0)) * (1.0 / (d * d));
  DirKu o;
  o.r = ks * ((eix * eix) * ui + (eix * ejx) * uj) + ks * ((eix * ekx) * uk);
  o.z = ks * ((eiy * eiy) * ui + (eiy * ejy) * uj) + ks * ((eiy * eky) * uk);
  return o;
}

// k_tangent_load's sibling for columns in k_r and k_z of anisotropic materials (same lists, staging, LDS carve-up and launch
// geometry): F[i * NV + j] = -sum over the triangles e at node i of (w_r (K_e^r u)_i if c_r(tag) = j) + (w_z (K_e^z u)_i if
// c_z(tag) = j), the table `dir` by tag-dictionary index in static LDS.  A visit whose tag has c_r == c_z and w_r == w_z is the
// isotropic product of k_tangent_load times w, so a set-up of kappa columns on tags with multipliers (1, 1) gives its bits.
// Each column's sum runs in list order in a register of the row's lane - no atomics, bitwise reproducible; columns nothing maps
// to are written as zeros.
template <int NV>
__global__ __launch_bounds__(RBA) void k_tangent_load_dir(int nblk, int capd, const int4* __restrict__ hdr, const uint4* __restrict__ ell,
                                                          const uint4* __restrict__ cid16, const double2* __restrict__ zrb,
                                                          const int32_t* __restrict__ dict, const int32_t* __restrict__ rowptr,
                                                          const TanDir* __restrict__ dir, const double* __restrict__ u,
                                                          double* __restrict__ F) {
  extern __shared__ double smem[];
  __shared__ TanDir sdir[64];
  double2* sXd = reinterpret_cast<double2*>(smem);
  double* sU = smem + 2 * capd;
  int* sR = reinterpret_cast<int*>(sU + capd + (capd & 1));
  uint4* sC4 = reinterpret_cast<uint4*>(sR + RBA + 4);
  const uint16_t* sC = reinterpret_cast<const uint16_t*>(sC4);
  const int t = threadIdx.x;
  if (t < 64) sdir[t] = dir[t];
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int4 cA = hdr[2 * blk], cB = hdr[2 * blk + 1];
    const int c0 = cA.x >> 3, nc = ((cA.x + cA.y + 7) >> 3) - c0;
    for (int i = t; i < nc; i += RBA) sC4[i] = cid16[c0 + i];
    for (int i = t; i < cA.w; i += RBA) { sXd[i] = zrb[cA.z + i]; sU[i] = u[dict[cA.z + i]]; }
    if (t < cB.w) sR[t] = rowptr[blk * RBA + t] - cA.x;
    __syncthreads();
    if (t < cB.w) {
#pragma clang fp contract(off)
      const int sbase = sR[t] + (cA.x & 7);
      const int ci = cB.z + t;
      const double2 Pi = sXd[ci];
      const double ui = sU[ci];
      double acc[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] = 0.0;
      for (int g = 0; g < cB.y; ++g) {
        const uint4 ev = ell[cB.x + g * RBA + t];
        const unsigned w[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const unsigned e = (w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
          if (e == 0xFFFFu) continue;
          const TanDir td = sdir[e >> 10];
          if (td.c_r < 0 && td.c_z < 0) continue;
          const int pj = sC[sbase + (e & 31u)], pk = sC[sbase + ((e >> 5) & 31u)];
          int cr = td.c_r, cz = td.c_z;
          double ar, az;
          if (cr == cz && td.w_r == td.w_z) {
            const ElemRow r = element_row(Pi, sXd[pj], sXd[pk], 0.0, 1.0);
            ar = td.w_r * ((r.k0 * ui + r.k1 * sU[pj]) + r.k2 * sU[pk]);
            az = 0.0;
            cz = -1;
          } else {
            const DirKu k = element_dir_ku(Pi, sXd[pj], sXd[pk], ui, sU[pj], sU[pk]);
            ar = td.w_r * k.r;
            az = td.w_z * k.z;
          }
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            if (j == cr) acc[j] += ar;
            if (j == cz) acc[j] += az;
          }
        }
      }
      double* out = F + static_cast<size_t>(blk * RBA + t) * NV;
#pragma unroll
      for (int j = 0; j < NV; ++j) out[j] = -acc[j];
    }
    __syncthreads();
  }
}

// Shape columns of a tangent run (hf_tangent_set_shape): the nodes move along z with the velocity v of a column,
// the triangles stay.  With the letters of element_row_of (x = z, y = r), edot_a.x the difference of v over edge a, edot_a.y = 0:
//   D = e_j.x e_k.y - e_j.y e_k.x (signed twice-area),  Ddot = edot_j.x e_k.y - e_j.y edot_k.x,  delta = Ddot / D
//   Mdot_e = delta M_e,   Kdot_ab = -delta K_ab + ks k_r (edot_a.x e_b.x + e_a.x edot_b.x),  ks = area (rsum / 3) / d^2, d = |D|
// isotropic tags with k_r = k_z = kappa.  What one visit shares between the columns:
struct ShapeVisit {
  double mk;            // (M_e w)_me - (K_e u)_me: delta multiplies it
  double kk;            // ks k_r
  double inv_D;         // 1 / D
  double eix, ejx, ekx, ejy, eky;
};
__device__ __forceinline__ ShapeVisit shape_visit(const double2 Pi, const double2 Pj, const double2 Pk, double rho_c, double k_z, double k_r,
                                                  double ui, double uj, double uk, double wi, double wj, double wk) {
#pragma clang fp contract(off)
  const double eix = Pk.x - Pj.x, eiy = Pk.y - Pj.y;     // edge opposite "me"
  const double ejx = Pi.x - Pk.x, ejy = Pi.y - Pk.y;     // opposite next
  const double ekx = Pj.x - Pi.x, eky = Pj.y - Pi.y;     // opposite previous
  const double D = ejx * eky - ejy * ekx;
  const double d = fabs(D);
  const double rsum = sorted_sum3(Pi.y, Pj.y, Pk.y);
  const double area = 0.5 * d;
  const double ks = area * (rsum * (1.0 / 3.0)) * (1.0 / (d * d));
  const double ms30 = rho_c * area * (1.0 / 30.0), ms60 = rho_c * area * (1.0 / 60.0);
  const double k0 = ks * (k_r * (eix * eix) + k_z * (eiy * eiy));
  const double k1 = ks * (k_r * (eix * ejx) + k_z * (eiy * ejy));
  const double k2 = ks * (k_r * (eix * ekx) + k_z * (eiy * eky));
  const double m0 = ms30 * (2.0 * Pi.y + rsum);
  const double m1 = ms60 * (rsum + (Pi.y + Pj.y));
  const double m2 = ms60 * (rsum + (Pi.y + Pk.y));
  ShapeVisit o;
  o.mk = ((m0 * wi + m1 * wj) + m2 * wk) - ((k0 * ui + k1 * uj) + k2 * uk);
  o.kk = ks * k_r;
  o.inv_D = 1.0 / D;
  o.eix = eix; o.ejx = ejx; o.ekx = ekx; o.ejy = ejy; o.eky = eky;
  return o;
}

// (Kdot_e u)_me + (Mdot_e w)_me of one column from its velocities at the visit's three nodes
__device__ __forceinline__ double shape_term(const ShapeVisit& s, double vi, double vj, double vk, double ui, double uj, double uk) {
#pragma clang fp contract(off)
  const double dix = vk - vj, djx = vi - vk, dkx = vj - vi;
  const double delta = (djx * s.eky - s.ejy * dkx) * s.inv_D;
  const double g = (((dix * s.eix + s.eix * dix) * ui + (dix * s.ejx + s.eix * djx) * uj) + (dix * s.ekx + s.eix * dkx) * uk);
  return delta * s.mk + s.kk * g;
}

struct ShapeArgs {
  int32_t dst[4];       // F column of each shape slot
  int32_t nv;           // columns of F
  int32_t wmode;        // w: 0 = zero (no step taken), 1 = (u - un) / dtp (backward Euler), 2 = ((u - 4/3 un) + 1/3 um1) / dtp (BDF2)
  double dtp;           // dt (backward Euler), 2/3 dt (BDF2)
};

// k_tangent_load's sibling for shape columns (same lists, block staging and launch geometry): it adds
//   F[i * nv + dst[s]] -= sum over the triangles e at node i of (Kdot_e^s u)_i + (Mdot_e^s w)_i,   s < NS,
// to what the load kernel of the set-up wrote.  Next to the coordinates and u = u^{n+1} the block's column nodes get w (formed
// here from u, un = u^n and um1 = u^{n-1}) and their NS velocities (vz, interleaved by node).  kappa, rho_c and the multipliers
// (m_z, m_r; null = none set) by tag-dictionary index, as the assembly kernels read them.  Each slot's sum runs in list order in
// a register of the row's lane - no atomics, bitwise reproducible.  A triangle whose three velocities agree contributes an exact 0.
template <int NS>
struct VisitShape {
  static constexpr int NODE = 2, WIDE = NS;                // sU, sW, then the NS velocities of a node
  static constexpr bool OCC_GRID = true;
  static constexpr RgVariant ID = NS == 1 ? RG_SHAPE1 : NS == 2 ? RG_SHAPE2 : RG_SHAPE4;
  double *skr, *skz, *src;                                 // [64] k_r, k_z and rho_c by tag-dictionary index
  const double *kappa_idx, *rhoc_idx;
  const double2* an_idx;
  const double *u, *un, *um1, *vz;
  ShapeArgs a;
  double* F;
  struct Row { double ui, wi, vi[NS], acc[NS]; };
  __device__ __forceinline__ void tables(int t) const {
#pragma clang fp contract(off)
    const double kap = kappa_idx[t];
    const double2 m = an_idx ? an_idx[t] : make_double2(1.0, 1.0);
    skz[t] = m.x * kap;
    skr[t] = m.y * kap;
    src[t] = rhoc_idx[t];
  }
  __device__ __forceinline__ void node(const VisitLds& L, int i, double2, const int32_t* __restrict__ dict, int g) const {
    double *sU = L.sN, *sW = sU + L.capw(), *sV = sW + L.capw();
    const int node = dict[g];
    const double u1 = u[node];
    sU[i] = u1;
    sW[i] = step_rate(u1, un, um1, node, a.wmode, a.dtp);
#pragma unroll
    for (int s = 0; s < NS; ++s) sV[i * NS + s] = vz[static_cast<size_t>(node) * NS + s];
  }
  __device__ __forceinline__ Row begin(const VisitLds& L, int ci) const {
    const double *sU = L.sN, *sW = sU + L.capw(), *sV = sW + L.capw();
    Row r;
    r.ui = sU[ci];
    r.wi = sW[ci];
#pragma unroll
    for (int s = 0; s < NS; ++s) { r.vi[s] = sV[ci * NS + s]; r.acc[s] = 0.0; }
    return r;
  }
  __device__ __forceinline__ Row visit(const VisitLds& L, Row r, const double2 Pi, int tg, unsigned ij, unsigned ik) const {
#pragma clang fp contract(off)
    const double *sU = L.sN, *sW = sU + L.capw(), *sV = sW + L.capw();
    const int pj = L.sC[ij], pk = L.sC[ik];
    const double uj = sU[pj], uk = sU[pk];
    const ShapeVisit sv = shape_visit(Pi, L.sXd[pj], L.sXd[pk], src[tg], skz[tg], skr[tg], r.ui, uj, uk, r.wi, sW[pj], sW[pk]);
#pragma unroll
    for (int s = 0; s < NS; ++s) r.acc[s] += shape_term(sv, r.vi[s], sV[pj * NS + s], sV[pk * NS + s], r.ui, uj, uk);
    return r;
  }
  __device__ __forceinline__ void store(const Row& r, int row) const {
#pragma clang fp contract(off)
    double* out = F + static_cast<size_t>(row) * a.nv;
#pragma unroll
    for (int s = 0; s < NS; ++s) out[a.dst[s]] -= r.acc[s];
  }
};

template <int NS>
__global__ __launch_bounds__(RBA) void k_tangent_load_shape(int nblk, int capd, const int4* __restrict__ hdr, const uint4* __restrict__ ell,
                                                            const uint4* __restrict__ cid16, const double2* __restrict__ zrb,
                                                            const int32_t* __restrict__ dict, const int32_t* __restrict__ rowptr,
                                                            const double* __restrict__ kappa_idx, const double* __restrict__ rhoc_idx,
                                                            const double2* __restrict__ an_idx, const double* __restrict__ u,
                                                            const double* __restrict__ un, const double* __restrict__ um1,
                                                            const double* __restrict__ vz, ShapeArgs a, double* __restrict__ F) {
  extern __shared__ double smem[];
  __shared__ double skr[64], skz[64], src[64];
  rowgather_visit(nblk, capd, hdr, ell, cid16, zrb, dict, rowptr,
                  VisitShape<NS>{skr, skz, src, kappa_idx, rhoc_idx, an_idx, u, un, um1, vz, a, F}, smem);
}

// k_tangent_load's sibling for capacity columns (hf_tangent_set_capacity; same lists, LDS carve-up and launch
// geometry): F[i * NV + j] -= sum over the triangles e at node i whose tag gives its rho_c to column j (ccol[tag-dictionary
// index] = j) of (M^1_e w)_i, M^1_e the r-weighted element mass at rho_c = 1 (element_row, as k_source_load forms it).  No state is
// staged: where k_tangent_load stages u the block's column nodes get the step rate w, formed from u = u^{n+1}, un = u^n and
// um1 = u^{n-1} statement for statement as k_tangent_load_shape forms it, so a node's w has that kernel's bits.  It runs after the
// load kernel of the set-up and touches only the columns of `cmask` (bit j: some tag maps to column j).  Each column's sum runs in
// list order in a register of the row's lane - no atomics, bitwise reproducible.
template <int NV>
__global__ __launch_bounds__(RBA) void k_tangent_load_cap(int nblk, int capd, const int4* __restrict__ hdr, const uint4* __restrict__ ell,
                                                          const uint4* __restrict__ cid16, const double2* __restrict__ zrb,
                                                          const int32_t* __restrict__ dict, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ ccol, const double* __restrict__ u,
                                                          const double* __restrict__ un, const double* __restrict__ um1, int wmode,
                                                          double dtp, unsigned cmask, double* __restrict__ F) {
  extern __shared__ double smem[];
  __shared__ int scc[64];
  double2* sXd = reinterpret_cast<double2*>(smem);
  double* sW = smem + 2 * capd;
  int* sR = reinterpret_cast<int*>(sW + capd + (capd & 1));
  uint4* sC4 = reinterpret_cast<uint4*>(sR + RBA + 4);
  const uint16_t* sC = reinterpret_cast<const uint16_t*>(sC4);
  const int t = threadIdx.x;
  if (t < 64) scc[t] = ccol[t];
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int4 cA = hdr[2 * blk], cB = hdr[2 * blk + 1];
    const int c0 = cA.x >> 3, nc = ((cA.x + cA.y + 7) >> 3) - c0;
    for (int i = t; i < nc; i += RBA) sC4[i] = cid16[c0 + i];
    for (int i = t; i < cA.w; i += RBA) {
#pragma clang fp contract(off)
      const int node = dict[cA.z + i];
      const double u1 = u[node];
      sXd[i] = zrb[cA.z + i];
      double w = 0.0;
      if (wmode == 1) w = (u1 - un[node]) / dtp;
      else if (wmode == 2) w = ((u1 - (4.0 / 3.0) * un[node]) + (1.0 / 3.0) * um1[node]) / dtp;
      sW[i] = w;
    }
    if (t < cB.w) sR[t] = rowptr[blk * RBA + t] - cA.x;
    __syncthreads();
    if (t < cB.w) {
#pragma clang fp contract(off)
      const int sbase = sR[t] + (cA.x & 7);
      const int ci = cB.z + t;
      const double2 Pi = sXd[ci];
      const double wi = sW[ci];
      double acc[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] = 0.0;
      for (int g = 0; g < cB.y; ++g) {
        const uint4 ev = ell[cB.x + g * RBA + t];
        const unsigned w[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const unsigned e = (w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
          if (e == 0xFFFFu) continue;
          const int cj = scc[e >> 10];
          if (cj < 0) continue;
          const int pj = sC[sbase + (e & 31u)], pk = sC[sbase + ((e >> 5) & 31u)];
          const ElemRow r = element_row(Pi, sXd[pj], sXd[pk], 1.0, 0.0);
          const double mw = (r.m0 * wi + r.m1 * sW[pj]) + r.m2 * sW[pk];
#pragma unroll
          for (int j = 0; j < NV; ++j)
            if (j == cj) acc[j] += mw;
        }
      }
      double* out = F + static_cast<size_t>(blk * RBA + t) * NV;
#pragma unroll
      for (int j = 0; j < NV; ++j)
        if ((cmask >> j) & 1u) out[j] -= acc[j];
    }
    __syncthreads();
  }
}

// Shape of the volumetric source (hf_set_source) at a node P = (z, r): s = exp(-(c_r r^2 + |z - z0| inv_depth)),
// c_r = 4 ln2 / fwhm^2 and inv_depth = 1 / depth, both formed on the host (inv_depth = 0: uniform through the layer).
// One double-precision exp per node; the argument is formed without contraction, so it has the bits of its restatement.
__device__ __forceinline__ double source_shape(const double2 P, double c_r, double z0, double inv_depth) {
#pragma clang fp contract(off)
  const double x = c_r * (P.y * P.y) + fabs(P.x - z0) * inv_depth;
  return exp(-x);
}

// Load of the volumetric source by row gather (k_tangent_load's lists, staging, LDS carve-up):
// F[i] = sum over the triangles e at node i whose tag absorbs (absorb[tag-dictionary index] != 0) of (M_e s)_i, M_e the
// r-weighted element mass at rho_c = 1 (element_row) and s the source shape at the element's three nodes, i.e. the P1
// interpolant of s inside each absorbing element, cut off at the material boundary.  No state is staged: where
// k_tangent_load stages u the block's column nodes get s, computed once per node from the staged coordinates, so every lane
// that reads a node sees the same bits.  The sum runs in list order in a register of the row's lane - no atomics, bitwise
// reproducible; rows with no absorbing triangle are written as zeros.
struct VisitSource {
  static constexpr int NODE = 1, WIDE = 0;                 // sS: the source shape
  static constexpr bool OCC_GRID = true;
  static constexpr RgVariant ID = RG_SOURCE;
  int* sabs;                                               // [64] absorbs or not, by tag-dictionary index
  const int32_t* absorb;
  double c_r, z0, inv_depth;
  double* F;
  struct Row { double si, acc; };
  __device__ __forceinline__ void tables(int t) const { sabs[t] = absorb[t]; }
  __device__ __forceinline__ void node(const VisitLds& L, int i, const double2 P, const int32_t*, int) const {
    L.sN[i] = source_shape(P, c_r, z0, inv_depth);
  }
  __device__ __forceinline__ Row begin(const VisitLds& L, int ci) const { return Row{L.sN[ci], 0.0}; }
  __device__ __forceinline__ Row visit(const VisitLds& L, Row r, const double2 Pi, int tg, unsigned ij, unsigned ik) const {
#pragma clang fp contract(off)
    const double* sS = L.sN;
    if (sabs[tg] == 0) return r;
    const int pj = L.sC[ij], pk = L.sC[ik];
    const ElemRow e = element_row(Pi, L.sXd[pj], L.sXd[pk], 1.0, 0.0);
    r.acc += (e.m0 * r.si + e.m1 * sS[pj]) + e.m2 * sS[pk];
    return r;
  }
  __device__ __forceinline__ void store(const Row& r, int row) const { F[row] = r.acc; }
};

__global__ __launch_bounds__(RBA) void k_source_load(int nblk, int capd, const int4* __restrict__ hdr, const uint4* __restrict__ ell,
                                                     const uint4* __restrict__ cid16, const double2* __restrict__ zrb,
                                                     const int32_t* __restrict__ rowptr, const int32_t* __restrict__ absorb,
                                                     double c_r, double z0, double inv_depth, double* __restrict__ F) {
  extern __shared__ double smem[];
  __shared__ int sabs[64];
  rowgather_visit(nblk, capd, hdr, ell, cid16, zrb, nullptr, rowptr, VisitSource{sabs, absorb, c_r, z0, inv_depth, F}, smem);
}

// k_source_load's sibling for a differentiable source (hf_source_derivatives; same lists, staging and launch
// geometry): G_f = dF1/dfwhm and G_d = dF1/ddepth, the unit-capacity element mass applied to the nodal values
//   s_f = s (2 c_r r^2 / fwhm)   and   s_d = s |z - z0| inv_depth^2   (0 for a uniform layer, inv_depth = 0)
// inside the absorbing elements, exactly as k_source_load forms F1 from s.  In one pass the block's column nodes get s_f and s_d
// from one s (s itself enters no sum and is not staged: one double per column node more LDS than k_source_load), each computed
// once per node, so every lane that reads a node sees the same bits.
// Each sum runs in list order in a register of the row's lane - no atomics, bitwise reproducible; rows with no absorbing
// triangle are written as exact zeros, and `has` gets 1 for a row with an absorbing triangle, 0 otherwise.
__global__ __launch_bounds__(RBA) void k_source_load_d(int nblk, int capd, const int4* __restrict__ hdr, const uint4* __restrict__ ell,
                                                       const uint4* __restrict__ cid16, const double2* __restrict__ zrb,
                                                       const int32_t* __restrict__ rowptr, const int32_t* __restrict__ absorb,
                                                       double c_r, double z0, double inv_depth, double fwhm,
                                                       double* __restrict__ Gf, double* __restrict__ Gd, int32_t* __restrict__ has) {
  extern __shared__ double smem[];
  __shared__ int sabs[64];
  const int capw = capd + (capd & 1);
  double2* sXd = reinterpret_cast<double2*>(smem);
  double* sF = smem + 2 * capd;
  double* sD = sF + capw;
  int* sR = reinterpret_cast<int*>(sD + capw);
  uint4* sC4 = reinterpret_cast<uint4*>(sR + RBA + 4);
  const uint16_t* sC = reinterpret_cast<const uint16_t*>(sC4);
  const int t = threadIdx.x;
  if (t < 64) sabs[t] = absorb[t];
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int4 cA = hdr[2 * blk], cB = hdr[2 * blk + 1];
    const int c0 = cA.x >> 3, nc = ((cA.x + cA.y + 7) >> 3) - c0;
    for (int i = t; i < nc; i += RBA) sC4[i] = cid16[c0 + i];
    for (int i = t; i < cA.w; i += RBA) {
#pragma clang fp contract(off)
      const double2 P = zrb[cA.z + i];
      const double s = source_shape(P, c_r, z0, inv_depth);
      sXd[i] = P;
      sF[i] = s * (((2.0 * c_r) * (P.y * P.y)) / fwhm);
      sD[i] = s * ((fabs(P.x - z0) * inv_depth) * inv_depth);
    }
    if (t < cB.w) sR[t] = rowptr[blk * RBA + t] - cA.x;
    __syncthreads();
    if (t < cB.w) {
#pragma clang fp contract(off)
      const int sbase = sR[t] + (cA.x & 7);
      const int ci = cB.z + t;
      const double2 Pi = sXd[ci];
      const double fi = sF[ci], di = sD[ci];
      double accf = 0.0, accd = 0.0;
      int any = 0;
      for (int g = 0; g < cB.y; ++g) {
        const uint4 ev = ell[cB.x + g * RBA + t];
        const unsigned w[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const unsigned e = (w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
          if (e == 0xFFFFu) continue;
          if (sabs[e >> 10] == 0) continue;
          const int pj = sC[sbase + (e & 31u)], pk = sC[sbase + ((e >> 5) & 31u)];
          const ElemRow r = element_row(Pi, sXd[pj], sXd[pk], 1.0, 0.0);
          accf += (r.m0 * fi + r.m1 * sF[pj]) + r.m2 * sF[pk];
          accd += (r.m0 * di + r.m1 * sD[pj]) + r.m2 * sD[pk];
          any = 1;
        }
      }
      Gf[blk * RBA + t] = accf;
      Gd[blk * RBA + t] = accd;
      has[blk * RBA + t] = any;
    }
    __syncthreads();
  }
}

// F0 + p F1: the load of a step when a source (hf_set_source) acts on top of a load (hf_set_load / hf_hold_load)
__global__ __launch_bounds__(TPB) void k_source_sum(int n, const double* __restrict__ F0, double p, const double* __restrict__ F1,
                                                    double* __restrict__ out) {
#pragma clang fp contract(off)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = F0[i] + p * F1[i];
}

// kappa(T) of one table (KTab): s = (T - t0) / dT, clamped to the end values, else v_i + (s - i) (v_{i+1} - v_i), i = floor(s)
__device__ __forceinline__ double ktab_eval(const KTab h, const double* __restrict__ vals, double T) {
#pragma clang fp contract(off)
  const double s = (T - h.t0) * h.inv_dt;
  if (!(s > 0.0)) return vals[h.off];
  if (s >= static_cast<double>(h.n - 1)) return vals[h.off + h.n - 1];
  const int i = min(static_cast<int>(s), h.n - 2);
  const double a = vals[h.off + i], b = vals[h.off + i + 1];
  return a + (s - static_cast<double>(i)) * (b - a);
}

// The table policies (hf_set_kappa_tables, hf_set_rhoc_tables, hf_steady_picard_setup) stage the block's slice of an evaluation
// state u* next to the coordinates, as k_grad_rows stages u.  Per triangle T_e = ((lo + mid) + hi) / 3 of its three sorted nodal
// values - the same bits from each vertex's point of view, so the operators stay exactly symmetric - and a coefficient is
// table(T_e) for a tabled tag (header n > 0, headers in static LDS), the constant by tag-dictionary index otherwise: constant
// tables give the bits of k_assemble_rows.
__device__ __forceinline__ double element_temperature(const double* sU, double ui, int cj, int ck) {
#pragma clang fp contract(off)
  return sorted_sum3(ui, sU[cj], sU[ck]) * (1.0 / 3.0);
}

// u* = u, or 2 u - uprev when uprev is given (BDF2's extrapolated state)
struct EvalState {
  const double *u, *uprev;
  __device__ __forceinline__ double operator()(int node) const {
#pragma clang fp contract(off)
    return uprev ? 2.0 * u[node] - uprev[node] : u[node];
  }
};

// d table / dT at T: the slope of the segment ktab_eval takes, branch for branch; 0 in both clamped ranges
__device__ __forceinline__ double ktab_slope(const KTab h, const double* __restrict__ vals, double T) {
#pragma clang fp contract(off)
  const double s = (T - h.t0) * h.inv_dt;
  if (!(s > 0.0)) return 0.0;
  if (s >= static_cast<double>(h.n - 1)) return 0.0;
  const int i = min(static_cast<int>(s), h.n - 2);
  return (vals[h.off + i + 1] - vals[h.off + i]) * h.inv_dt;
}

// k_tangent_load_cap's sibling for tangent runs under kappa(T) / rho_c(T) tables (hf_table_derivatives; same lists,
// block staging and launch geometry).  On every triangle e of a tabled tag, with T_e the element temperature of the evaluation state
// u* the primal step valued its operators at (element_temperature: the assembly's bits) and sigma_j = the mean of column j's s* over
// the triangle's nodes (s* formed from s^n, s^{n-1} as u* from u^n, u^{n-1}),
//   F[i * NV + j] -= kdot_j (K^1_e u)_i + cdot_j (M^1_e w)_i,
//   kdot_j = D^k_{j,tag}(T_e) + kappa'_tag(T_e) sigma_j,   cdot_j = D^c_{j,tag}(T_e) + rho_c'_tag(T_e) sigma_j,
// K^1_e and M^1_e the element matrices at unit coefficients (one element_row), u = u^{n+1} and w the step rate as
// k_tangent_load_cap forms it.  D: a derivative table on the tag's own grid (hf_tangent_set_tables), found through koff / coff
// ([64][NV] offsets into dkvals / dcvals by tag-dictionary index and column, -1 = none; a null array: none of that kind) and evaluated by ktab_eval.  Next to the
// coordinates the block's column nodes get u, w, u* and the NV values of s*.  Triangles of untabled tags are skipped before any
// arithmetic, rows that meet none are not written.  Each column's sum runs in list order in a register of the row's lane - no
// atomics, bitwise reproducible.  ctab == nullptr: no capacity tables.
template <int NV>
__global__ __launch_bounds__(RBA) void k_tangent_load_T(int nblk, int capd, const int4* __restrict__ hdr, const uint4* __restrict__ ell,
                                                        const uint4* __restrict__ cid16, const double2* __restrict__ zrb,
                                                        const int32_t* __restrict__ dict, const int32_t* __restrict__ rowptr,
                                                        const KTab* __restrict__ ktab, const double* __restrict__ kvals,
                                                        const KTab* __restrict__ ctab, const double* __restrict__ cvals,
                                                        const int32_t* __restrict__ koff, const double* __restrict__ dkvals,
                                                        const int32_t* __restrict__ coff, const double* __restrict__ dcvals,
                                                        const double* __restrict__ u, const double* __restrict__ un,
                                                        const double* __restrict__ um1, int wmode, double dtp, EvalState state,
                                                        const double* __restrict__ s, const double* __restrict__ sprev,
                                                        double* __restrict__ F) {
  extern __shared__ double smem[];
  __shared__ KTab sK[64], sCt[64];
  const int capw = capd + (capd & 1);
  double2* sXd = reinterpret_cast<double2*>(smem);
  double* sU = smem + 2 * capd;
  double* sW = sU + capw;
  double* sE = sW + capw;
  double* sS = sE + capw;
  int* sR = reinterpret_cast<int*>(sS + static_cast<size_t>(capd) * NV);
  uint4* sC4 = reinterpret_cast<uint4*>(sR + RBA + 4);
  const uint16_t* sC = reinterpret_cast<const uint16_t*>(sC4);
  const int t = threadIdx.x;
  if (t < 64) {
    sK[t] = ktab[t];
    sCt[t] = ctab ? ctab[t] : KTab{0.0, 0.0, 0, 0};
  }
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int4 cA = hdr[2 * blk], cB = hdr[2 * blk + 1];
    const int c0 = cA.x >> 3, nc = ((cA.x + cA.y + 7) >> 3) - c0;
    for (int i = t; i < nc; i += RBA) sC4[i] = cid16[c0 + i];
    for (int i = t; i < cA.w; i += RBA) {
#pragma clang fp contract(off)
      const int node = dict[cA.z + i];
      const double u1 = u[node];
      sXd[i] = zrb[cA.z + i];
      sU[i] = u1;
      double w = 0.0;
      if (wmode == 1) w = (u1 - un[node]) / dtp;
      else if (wmode == 2) w = ((u1 - (4.0 / 3.0) * un[node]) + (1.0 / 3.0) * um1[node]) / dtp;
      sW[i] = w;
      sE[i] = state(node);
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const double sj = s[static_cast<size_t>(node) * NV + j];
        sS[i * NV + j] = sprev ? 2.0 * sj - sprev[static_cast<size_t>(node) * NV + j] : sj;
      }
    }
    if (t < cB.w) sR[t] = rowptr[blk * RBA + t] - cA.x;
    __syncthreads();
    if (t < cB.w) {
#pragma clang fp contract(off)
      const int sbase = sR[t] + (cA.x & 7);
      const int ci = cB.z + t;
      const double2 Pi = sXd[ci];
      const double ui = sU[ci], wi = sW[ci], ei = sE[ci];
      double acc[NV];
#pragma unroll
      for (int j = 0; j < NV; ++j) acc[j] = 0.0;
      bool any = false;
      for (int g = 0; g < cB.y; ++g) {
        const uint4 ev = ell[cB.x + g * RBA + t];
        const unsigned w[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const unsigned e = (w[q >> 1] >> ((q & 1) * 16)) & 0xFFFFu;
          if (e == 0xFFFFu) continue;
          const int tg = e >> 10;
          const KTab kh = sK[tg], ch = sCt[tg];
          if (kh.n <= 0 && ch.n <= 0) continue;
          any = true;
          const int pj = sC[sbase + (e & 31u)], pk = sC[sbase + ((e >> 5) & 31u)];
          const double Te = element_temperature(sE, ei, pj, pk);
          const ElemRow r = element_row(Pi, sXd[pj], sXd[pk], 1.0, 1.0);
          const double ku = (r.k0 * ui + r.k1 * sU[pj]) + r.k2 * sU[pk];
          const double mw = (r.m0 * wi + r.m1 * sW[pj]) + r.m2 * sW[pk];
          const double kslope = kh.n > 0 ? ktab_slope(kh, kvals, Te) : 0.0;
          const double cslope = ch.n > 0 ? ktab_slope(ch, cvals, Te) : 0.0;
#pragma unroll
          for (int j = 0; j < NV; ++j) {
            const double sigma = ((sS[ci * NV + j] + sS[pj * NV + j]) + sS[pk * NV + j]) * (1.0 / 3.0);
            double kd = kslope * sigma, cd = cslope * sigma;
            if (kh.n > 0) {
              const int o = koff ? koff[tg * NV + j] : -1;
              if (o >= 0) kd += ktab_eval(KTab{kh.t0, kh.inv_dt, kh.n, o}, dkvals, Te);
            }
            if (ch.n > 0) {
              const int o = coff ? coff[tg * NV + j] : -1;
              if (o >= 0) cd += ktab_eval(KTab{ch.t0, ch.inv_dt, ch.n, o}, dcvals, Te);
            }
            acc[j] += kd * ku + cd * mw;
          }
        }
      }
      if (any) {
        double* out = F + static_cast<size_t>(blk * RBA + t) * NV;
#pragma unroll
        for (int j = 0; j < NV; ++j) out[j] -= acc[j];
      }
    }
    __syncthreads();
  }
}

// The coefficient policy of the six table kernels, one yes/no choice per axis:
//   CAP  a capacity table next to the conductivity table (k_assemble_rows_cT, _cT_an; launched only while a capacity table is
//        set): a second header array sCt for rho_c and the (M, A) slab, M = M(rho_c(T)) and A = M + dt K(kappa(T)) at u*, both
//        arrays written.  T_e is computed once per element visit - when either coefficient of the tag carries a table - and
//        used for both.  Not CAP: a one-value slab; M does not change, only A (or K) is written; sCt and cvals are not used.
//   K    the stiffness alone, K = K(kappa(T)) at the state u (k_assemble_rows_kT_K, _kT_K_an; hf_steady_picard_setup /
//        hf_steady_picard_solve): no M, no dt, rho_c = 0, the state is u itself (uprev, rhoc_idx and dt are not used).  With no
//        table (every header n = 0) or constant tables it gives the K of k_assemble_rows<true> bit for bit.  Not with CAP.
//   AN   the (m_z, m_r) multipliers on anisotropic tags (the three *_an kernels; hf_set_aniso_tables; launched only while a tag
//        is anisotropic and tables are set - kt_revalue, steady_revalue): kappa (and rho_c) are found exactly as without AN - the
//        same T_e, the same table evaluation - and the element routine is then chosen as RowsConst<K, true>::row chooses it,
//        with an_idx[tg] = (m_z, m_r): k_z = m_z kappa(T_e), k_r = m_r kappa(T_e), rho_c untouched.  So with every multiplier 1
//        an *_an kernel gives its sibling's bits, with constant tables those of k_assemble_rows_an, and in a mixed mesh a row
//        that touches only tags with m_z == m_r keeps the bits of the isotropic table kernel.  Not AN: an_idx is not used.
// The flags, hence LDS carve-up and footprint, depend on (CAP, K) alone.  Every instantiation compiles to the machine code its
// kernel had under a struct of its own (profiles/rows_table_asm_compare.txt).
template <bool CAP, bool K, bool AN>
struct RowsTable {
  static_assert(!(CAP && K), "no stiffness-only kernel with a capacity table");
  static constexpr bool PAIR = CAP, STATE = true, KONLY = K, NODE_FIRST = !K;
  static constexpr RgVariant ID = AN ? (CAP ? RG_CT_AN : K ? RG_KT_K_AN : RG_KT_AN) : (CAP ? RG_CT : K ? RG_KT_K : RG_KT);
  const KTab *sK, *sCt;
  const double *kvals, *cvals, *kappa_idx, *rhoc_idx;
  const double2* an_idx;
  double dt;
  EvalState ustar;
  __device__ __forceinline__ double state(int node) const {
    if constexpr (K) return ustar.u[node];
    else return ustar(node);
  }
  __device__ __forceinline__ ElemRow row(int tg, const double2 Pi, const double2 Pj, const double2 Pk, const double* sU, double ui, int cj,
                                         int ck) const {
    const KTab kh = sK[tg];
    double kappa = kappa_idx[tg], rho_c = 0.0;
    if constexpr (CAP) {
      const KTab ch = sCt[tg];
      rho_c = rhoc_idx[tg];
      if (kh.n > 0 || ch.n > 0) {
        const double Te = element_temperature(sU, ui, cj, ck);
        if (kh.n > 0) kappa = ktab_eval(kh, kvals, Te);
        if (ch.n > 0) rho_c = ktab_eval(ch, cvals, Te);
      }
    } else {
      if (kh.n > 0) kappa = ktab_eval(kh, kvals, element_temperature(sU, ui, cj, ck));
      if constexpr (!K) rho_c = rhoc_idx[tg];
    }
    if constexpr (AN) return element_row_m(Pi, Pj, Pk, rho_c, kappa, an_idx[tg]);
    else return element_row(Pi, Pj, Pk, rho_c, kappa);
  }
};

__global__ __launch_bounds__(RBA) void k_assemble_rows_kT(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                          const int32_t* __restrict__ rowptr, const int4* __restrict__ hdr,
                                                          const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                          const double2* __restrict__ zrb, const int32_t* __restrict__ dict,
                                                          const KTab* __restrict__ ktab, const double* __restrict__ kvals,
                                                          const double* __restrict__ kappa_idx, const double* __restrict__ rhoc_idx,
                                                          double dt, const double* __restrict__ u, const double* __restrict__ uprev,
                                                          double* __restrict__ Av) {
  extern __shared__ double smem[];
  __shared__ KTab sK[64];
  if (threadIdx.x < 64) sK[threadIdx.x] = ktab[threadIdx.x];
  rowgather_assemble(nblk, cap, capd, rowptr, hdr, ell, cid16, zrb, dict,
                     RowsTable<false, false, false>{sK, nullptr, kvals, nullptr, kappa_idx, rhoc_idx, nullptr, dt, {u, uprev}}, nullptr, Av, smem);
}

__global__ __launch_bounds__(RBA) void k_assemble_rows_cT(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                          const int32_t* __restrict__ rowptr, const int4* __restrict__ hdr,
                                                          const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                          const double2* __restrict__ zrb, const int32_t* __restrict__ dict,
                                                          const KTab* __restrict__ ktab, const double* __restrict__ kvals,
                                                          const KTab* __restrict__ ctab, const double* __restrict__ cvals,
                                                          const double* __restrict__ kappa_idx, const double* __restrict__ rhoc_idx,
                                                          double dt, const double* __restrict__ u, const double* __restrict__ uprev,
                                                          double* __restrict__ Mv, double* __restrict__ Av) {
  extern __shared__ double smem[];
  __shared__ KTab sK[64], sCt[64];
  if (threadIdx.x < 64) { sK[threadIdx.x] = ktab[threadIdx.x]; sCt[threadIdx.x] = ctab[threadIdx.x]; }
  rowgather_assemble(nblk, cap, capd, rowptr, hdr, ell, cid16, zrb, dict,
                     RowsTable<true, false, false>{sK, sCt, kvals, cvals, kappa_idx, rhoc_idx, nullptr, dt, {u, uprev}}, Mv, Av, smem);
}

__global__ __launch_bounds__(RBA) void k_assemble_rows_kT_K(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                            const int32_t* __restrict__ rowptr, const int4* __restrict__ hdr,
                                                            const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                            const double2* __restrict__ zrb, const int32_t* __restrict__ dict,
                                                            const KTab* __restrict__ ktab, const double* __restrict__ kvals,
                                                            const double* __restrict__ kappa_idx, const double* __restrict__ u,
                                                            double* __restrict__ Kv) {
  extern __shared__ double smem[];
  __shared__ KTab sK[64];
  if (threadIdx.x < 64) sK[threadIdx.x] = ktab[threadIdx.x];
  rowgather_assemble(nblk, cap, capd, rowptr, hdr, ell, cid16, zrb, dict,
                     RowsTable<false, true, false>{sK, nullptr, kvals, nullptr, kappa_idx, nullptr, nullptr, 0.0, {u, nullptr}}, nullptr, Kv, smem);
}

__global__ __launch_bounds__(RBA) void k_assemble_rows_kT_an(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                             const int32_t* __restrict__ rowptr, const int4* __restrict__ hdr,
                                                             const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                             const double2* __restrict__ zrb, const int32_t* __restrict__ dict,
                                                             const KTab* __restrict__ ktab, const double* __restrict__ kvals,
                                                             const double* __restrict__ kappa_idx, const double* __restrict__ rhoc_idx,
                                                             const double2* __restrict__ an_idx /* (m_z, m_r) */,
                                                             double dt, const double* __restrict__ u, const double* __restrict__ uprev,
                                                             double* __restrict__ Av) {
  extern __shared__ double smem[];
  __shared__ KTab sK[64];
  if (threadIdx.x < 64) sK[threadIdx.x] = ktab[threadIdx.x];
  rowgather_assemble(nblk, cap, capd, rowptr, hdr, ell, cid16, zrb, dict,
                     RowsTable<false, false, true>{sK, nullptr, kvals, nullptr, kappa_idx, rhoc_idx, an_idx, dt, {u, uprev}}, nullptr, Av, smem);
}

__global__ __launch_bounds__(RBA) void k_assemble_rows_cT_an(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                             const int32_t* __restrict__ rowptr, const int4* __restrict__ hdr,
                                                             const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                             const double2* __restrict__ zrb, const int32_t* __restrict__ dict,
                                                             const KTab* __restrict__ ktab, const double* __restrict__ kvals,
                                                             const KTab* __restrict__ ctab, const double* __restrict__ cvals,
                                                             const double* __restrict__ kappa_idx, const double* __restrict__ rhoc_idx,
                                                             const double2* __restrict__ an_idx /* (m_z, m_r) */,
                                                             double dt, const double* __restrict__ u, const double* __restrict__ uprev,
                                                             double* __restrict__ Mv, double* __restrict__ Av) {
  extern __shared__ double smem[];
  __shared__ KTab sK[64], sCt[64];
  if (threadIdx.x < 64) { sK[threadIdx.x] = ktab[threadIdx.x]; sCt[threadIdx.x] = ctab[threadIdx.x]; }
  rowgather_assemble(nblk, cap, capd, rowptr, hdr, ell, cid16, zrb, dict,
                     RowsTable<true, false, true>{sK, sCt, kvals, cvals, kappa_idx, rhoc_idx, an_idx, dt, {u, uprev}}, Mv, Av, smem);
}

__global__ __launch_bounds__(RBA) void k_assemble_rows_kT_K_an(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                               const int32_t* __restrict__ rowptr, const int4* __restrict__ hdr,
                                                               const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                               const double2* __restrict__ zrb, const int32_t* __restrict__ dict,
                                                               const KTab* __restrict__ ktab, const double* __restrict__ kvals,
                                                               const double* __restrict__ kappa_idx,
                                                               const double2* __restrict__ an_idx /* (m_z, m_r) */,
                                                               const double* __restrict__ u, double* __restrict__ Kv) {
  extern __shared__ double smem[];
  __shared__ KTab sK[64];
  if (threadIdx.x < 64) sK[threadIdx.x] = ktab[threadIdx.x];
  rowgather_assemble(nblk, cap, capd, rowptr, hdr, ell, cid16, zrb, dict,
                     RowsTable<false, true, true>{sK, nullptr, kvals, nullptr, kappa_idx, nullptr, an_idx, 0.0, {u, nullptr}}, nullptr, Kv, smem);
}

// The mean of the clamped piecewise-linear table over [min, max] of Ta and Tb (symmetric in them), for the enthalpy form of the
// capacity (hf_set_capacity_form).  Everything in knot units s = (T - t0) / dT.  Both ends in one segment, or in
// one clamped range: the table at the midpoint - exact for a linear piece, no cancellation as Tb -> Ta, and ktab_eval's own
// arithmetic at Ta == Tb.  Otherwise (first partial piece as length x midpoint value + cum[j] - cum[i] of the whole segments
// between + last partial piece) / (max - min); cum[j] = sum_{i < j} (v_i + v_{i+1}) / 2, the cumulative trapezoids per knot
// (built on the host, the layout of vals).
__device__ __forceinline__ double ktab_mean(const KTab h, const double* __restrict__ vals, const double* __restrict__ cum, double Ta,
                                            double Tb) {
#pragma clang fp contract(off)
  const double sl = (fmin(Ta, Tb) - h.t0) * h.inv_dt, sh = (fmax(Ta, Tb) - h.t0) * h.inv_dt;
  const double top = static_cast<double>(h.n - 1);
  if (!(sh > 0.0)) return vals[h.off];
  if (sl >= top) return vals[h.off + h.n - 1];
  const bool below = !(sl > 0.0), above = sh >= top;
  const int il = below ? 0 : min(static_cast<int>(sl), h.n - 2);
  const int ih = above ? h.n - 1 : min(static_cast<int>(sh), h.n - 2);
  if (!below && !above && il == ih) {
    const double a = vals[h.off + il], b = vals[h.off + il + 1];
    const double sm = sl + 0.5 * (sh - sl);
    return a + (sm - static_cast<double>(il)) * (b - a);
  }
  double head, tail;
  int jl;
  if (below) {
    head = (0.0 - sl) * vals[h.off];
    jl = 0;
  } else {
    const double a = vals[h.off + il], b = vals[h.off + il + 1];
    const double x = sl - static_cast<double>(il);                  // in [0, 1): the piece runs from x to 1
    head = (1.0 - x) * (a + (0.5 * (x + 1.0)) * (b - a));
    jl = il + 1;
  }
  if (above) {
    tail = (sh - top) * vals[h.off + h.n - 1];
  } else {
    const double a = vals[h.off + ih], b = vals[h.off + ih + 1];
    const double x = sh - static_cast<double>(ih);                  // the piece runs from 0 to x
    tail = x * (a + (0.5 * x) * (b - a));
  }
  return ((head + (cum[h.off + ih] - cum[h.off + jl])) + tail) / (sh - sl);
}

// The r-weighted element temperature Tw_e = sum_j (rs + r_j) u_j / (4 rs), rs = r_0 + r_1 + r_2: the volume average of the P1 field
// (k_monitor's I1 / I0).  rs and the sum of the three products go through sorted_sum3, so the three rows that visit a triangle
// - and k_stored_heat - get the same bits.
__device__ __forceinline__ double element_tw(double r0, double r1, double r2, double u0, double u1, double u2) {
#pragma clang fp contract(off)
  const double rs = sorted_sum3(r0, r1, r2);
  return sorted_sum3((rs + r0) * u0, (rs + r1) * u1, (rs + r2) * u2) / (4.0 * rs);
}

// The coefficient policy of the enthalpy form (hf_set_capacity_form; k_assemble_rows_hT): RowsTable<true, false,
// false>'s slab, headers and conductivity (kappa = table(T_e) at the plain-mean T_e of the evaluation state e, sU), and a second
// staged state u^n (sU2): the capacity of a tabled tag is the chord value, the table's mean between Tw_e(u^n) and Tw_e(e)
// (ktab_mean; table(Tw_e) where they are equal), so that 1^T M (x - u^n) is the change of the stored heat when e = x.
struct RowsEnthalpy {
  static constexpr bool PAIR = true, STATE = true, STATE2 = true, KONLY = false, NODE_FIRST = true;
  static constexpr RgVariant ID = RG_HT;
  const KTab *sK, *sCt;
  const double *kvals, *cvals, *ccum, *kappa_idx, *rhoc_idx;
  double dt;
  const double *e, *un;
  __device__ __forceinline__ double state(int node) const { return e[node]; }
  __device__ __forceinline__ double state2(int node) const { return un[node]; }
  __device__ __forceinline__ ElemRow row(int tg, const double2 Pi, const double2 Pj, const double2 Pk, const double* sU, double ui,
                                         const double* sU2, double ui2, int cj, int ck) const {
    const KTab kh = sK[tg], ch = sCt[tg];
    double kappa = kappa_idx[tg], rho_c = rhoc_idx[tg];
    if (kh.n > 0) kappa = ktab_eval(kh, kvals, element_temperature(sU, ui, cj, ck));
    if (ch.n > 0) {
      const double Ta = element_tw(Pi.y, Pj.y, Pk.y, ui2, sU2[cj], sU2[ck]);
      const double Tb = element_tw(Pi.y, Pj.y, Pk.y, ui, sU[cj], sU[ck]);
      rho_c = ktab_mean(ch, cvals, ccum, Ta, Tb);
    }
    return element_row(Pi, Pj, Pk, rho_c, kappa);
  }
};

__global__ __launch_bounds__(RBA) void k_assemble_rows_hT(int nblk, int cap /* slab slots, even */, int capd /* column-list slots */,
                                                          const int32_t* __restrict__ rowptr, const int4* __restrict__ hdr,
                                                          const uint4* __restrict__ ell, const uint4* __restrict__ cid16,
                                                          const double2* __restrict__ zrb, const int32_t* __restrict__ dict,
                                                          const KTab* __restrict__ ktab, const double* __restrict__ kvals,
                                                          const KTab* __restrict__ ctab, const double* __restrict__ cvals,
                                                          const double* __restrict__ ccum,
                                                          const double* __restrict__ kappa_idx, const double* __restrict__ rhoc_idx,
                                                          double dt, const double* __restrict__ e, const double* __restrict__ un,
                                                          double* __restrict__ Mv, double* __restrict__ Av) {
  extern __shared__ double smem[];
  __shared__ KTab sK[64], sCt[64];
  if (threadIdx.x < 64) { sK[threadIdx.x] = ktab[threadIdx.x]; sCt[threadIdx.x] = ctab[threadIdx.x]; }
  rowgather_assemble(nblk, cap, capd, rowptr, hdr, ell, cid16, zrb, dict,
                     RowsEnthalpy{sK, sCt, kvals, cvals, ccum, kappa_idx, rhoc_idx, dt, e, un}, Mv, Av, smem);
}

// out = e + w (x - e): the relaxed evaluation state of the enthalpy form's next sweep (launched only when w < 1; out may be e)
__global__ __launch_bounds__(TPB) void k_relax(int n, const double* e, const double* __restrict__ x, double w, double* out) {
#pragma clang fp contract(off)
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    const double ei = e[i];
    out[i] = ei + w * (x[i] - ei);
  }
}

// w = u^n, or BDF2's operand (4 u^n - u^{n-1}) / 3: the vector the re-valued M multiplies in Picard sweeps 2..p of a step with
// capacity tables (kept before the right-hand side's pass of sweep 1 rotates the state buffers)
__global__ __launch_bounds__(TPB) void k_picard_w(int n, const double* __restrict__ u, const double* __restrict__ um1,
                                                  double* __restrict__ out) {
#pragma clang fp contract(off)
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) out[i] = um1 ? (4.0 * u[i] - um1[i]) * (1.0 / 3.0) : u[i];
}

// max |a - b| over n entries into *out (the bits of a double >= 0, which order as unsigned integers; *out zeroed before)
__global__ __launch_bounds__(TPB) void k_max_abs_diff(int n, const double* __restrict__ a, const double* __restrict__ b,
                                                      unsigned long long* __restrict__ out) {
  __shared__ double s[TPB];
  double m = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) m = fmax(m, fabs(a[i] - b[i]));
  s[threadIdx.x] = m;
  __syncthreads();
  for (int h = TPB / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(out, static_cast<unsigned long long>(__double_as_longlong(s[0])));
}

// u* = u, or 2 u - uprev (the evaluation state of k_assemble_rows_kT, kept for the Picard change)
__global__ __launch_bounds__(TPB) void k_eval_state(int n, const double* __restrict__ u, const double* __restrict__ uprev,
                                                    double* __restrict__ out) {
#pragma clang fp contract(off)
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) out[i] = uprev ? 2.0 * u[i] - uprev[i] : u[i];
}

// Variable-step BDF2 (hf_set_step), launched only on a step whose ratio w = dt_n / dt_{n-1} is not 1:
// k_picard_w_var: out = a u^n - b u^{n-1}, the operand of the right-hand side as k_spmv's VB instances stage it;
// k_eval_state_var: out = (1 + w) u^n - w u^{n-1}, the evaluation state of the table kernels.
__device__ __forceinline__ double bdf2_operand_var(double a, double b, double un, double unm1) {
#pragma clang fp contract(off)
  return a * un - b * unm1;
}
__global__ __launch_bounds__(TPB) void k_picard_w_var(int n, const double* __restrict__ u, const double* __restrict__ um1, double a, double b,
                                                      double* __restrict__ out) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) out[i] = bdf2_operand_var(a, b, u[i], um1[i]);
}
__global__ __launch_bounds__(TPB) void k_eval_state_var(int n, const double* __restrict__ u, const double* __restrict__ uprev, double w,
                                                        double* __restrict__ out) {
#pragma clang fp contract(off)
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) out[i] = (1.0 + w) * u[i] - w * uprev[i];
}

// Local-error indicator of the last step (hf_get_step_error): over the rows with free[i] != 0,
//   max_i |c (((u_i - w0 h0_i) - w1 h1_i) - w2 h2_i)| / (atol + rtol |u_i|)
// into *out as k_max_abs_diff leaves its maximum (the bits of a double >= 0 order as unsigned integers; *out zeroed before): the
// answer does not depend on the order in which the workgroups arrive.  h2 null: the term is left out (backward Euler).  A row whose
// quotient is NaN or infinite makes the result +inf.
__global__ __launch_bounds__(TPB) void k_step_error(int n, const double* __restrict__ u, const double* __restrict__ h0,
                                                    const double* __restrict__ h1, const double* __restrict__ h2, double w0, double w1,
                                                    double w2, double c, double atol, double rtol, const uint8_t* __restrict__ free_row,
                                                    unsigned long long* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double s[TPB];
  double m = 0.0;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    if (!free_row[i]) continue;
    const double ui = u[i];
    double d = (ui - w0 * h0[i]) - w1 * h1[i];
    if (h2) d = d - w2 * h2[i];
    const double q = fabs(c * d) / (atol + rtol * fabs(ui));
    // a state or quotient that is not finite must not vanish in fmax (which drops NaN): the step's indicator is +inf, whose bits
    // order above every finite value, and the caller rejects the step
    m = (q <= 1.7976931348623157e308) ? fmax(m, q) : __longlong_as_double(0x7ff0000000000000LL);
  }
  s[threadIdx.x] = m;
  __syncthreads();
  for (int h = TPB / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(out, static_cast<unsigned long long>(__double_as_longlong(s[0])));
}

// mask[dofs[q]] = 0 (the Dirichlet rows of k_step_error's row mask, which is set to 1 before)
__global__ void k_clear_bytes(int m, const int32_t* __restrict__ dofs, uint8_t* __restrict__ mask) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < m) mask[dofs[q]] = 0;
}

// per-block copy of the coordinates of each block's column list (hf_set_mesh, once)
__global__ void k_gather_coords(int64_t total, const int32_t* __restrict__ dict, const double2* __restrict__ zr,
                                double2* __restrict__ zrb) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < total) zrb[i] = zr[dict[i]];
}

// Baseline: one thread per element, f64 atomics into global CSR (values must be zeroed).
__global__ __launch_bounds__(TPB) void k_assemble_global(int ne, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ colidx,
                                                         const int4* __restrict__ elem,
                                                         const double2* __restrict__ zr,
                                                         const double* __restrict__ kappa_tab,
                                                         const double* __restrict__ rhoc_tab, double dt,
                                                         double* __restrict__ Mv, double* __restrict__ Av) {
  const int e = blockIdx.x * TPB + threadIdx.x;
  if (e >= ne) return;
  const int4 el = elem[e];
  const int nd[3] = {el.x, el.y, el.z};
  double m[6], kk[6], av6[6];
  element_local(zr[el.x], zr[el.y], zr[el.z], rhoc_tab[el.w], kappa_tab[el.w], m, kk);
#pragma unroll
  for (int q = 0; q < 6; ++q) av6[q] = fma(dt, kk[q], m[q]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int s0 = rowptr[nd[a]], s1 = rowptr[nd[a] + 1];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      int s = s0;
      while (s < s1 && colidx[s] != nd[b]) ++s;
      const int q = sym_index(a, b);
      atomicAdd(&Mv[s], m[q]);
      atomicAdd(&Av[s], av6[q]);
    }
  }
}

// ------------------------------------------------------------------------------------------
// Read-flux projection (reference run_no_diamond.py:479-489, 544-550): L2 projection of grad T
// onto vector P1 with the r-weighted mass matrix.  The reference solves one 2n x 2n system; the
// components decouple into two scalar solves with M_r(1).  This kernel forms both right-hand
// sides  b_c[i] = sum_e (d_c T)_e * int_e phi_i r dx,  int_e phi_i r = |K| (2 r_i + r_j + r_k)/12,
// owner-computes like the assembly: a workgroup owns RBA rows and adds the incident elements.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RBA) void k_grad_rhs(int n, const int32_t* __restrict__ blk_eptr,
                                                  const int2* __restrict__ blk_ent, const double2* __restrict__ zr,
                                                  const double* __restrict__ u, double* __restrict__ bz,
                                                  double* __restrict__ br) {
  __shared__ double sB[2 * RBA];
  const int blk = blockIdx.x;
  const int r0 = blk * RBA;
  const int r1 = min(n, r0 + RBA);
  for (int k = threadIdx.x; k < 2 * RBA; k += RBA) sB[k] = 0.0;
  __syncthreads();
  for (int q = blk_eptr[blk] + threadIdx.x; q < blk_eptr[blk + 1]; q += RBA) {
#pragma clang fp contract(off)
    const AsmEntry e = load_entry(blk_ent, q);
    const double2 p0 = zr[e.n0], p1 = zr[e.n1], p2 = zr[e.n2];
    const double u0 = u[e.n0], u1 = u[e.n1], u2 = u[e.n2];
    const double d = (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
    const double area = 0.5 * fabs(d);
    // grad phi_i = (b_i, c_i)/d
    const double gz = (u0 * (p1.y - p2.y) + u1 * (p2.y - p0.y) + u2 * (p0.y - p1.y)) / d;
    const double gr = (u0 * (p2.x - p1.x) + u1 * (p0.x - p2.x) + u2 * (p1.x - p0.x)) / d;
    const double rsum = (p0.y + p1.y) + p2.y;
    const double wgt[3] = {area * (p0.y + rsum) / 12.0, area * (p1.y + rsum) / 12.0, area * (p2.y + rsum) / 12.0};
    const int nd[3] = {e.n0, e.n1, e.n2};
    const unsigned owned = (e.w3 >> 8) & 7u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!((owned >> a) & 1u)) continue;
      atomicAdd(&sB[2 * (nd[a] - r0)], gz * wgt[a]);
      atomicAdd(&sB[2 * (nd[a] - r0) + 1], gr * wgt[a]);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < r1 - r0; k += RBA) {
    bz[r0 + k] = sB[2 * k];
    br[r0 + k] = sB[2 * k + 1];
  }
}

// ------------------------------------------------------------------------------------------
// Dirichlet elimination (what dolfinx assemble_matrix(form, bcs) leaves): BC rows and
// columns zeroed, unit diagonal.  The column entries A[i, j in B] of free rows i are saved
// first - they are the lifting operator of apply_lifting (run_with_diamond.py:477).
// ------------------------------------------------------------------------------------------
__global__ void k_take_lift(int nlift, const int32_t* __restrict__ slot, double* __restrict__ A,
                            double* __restrict__ val) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nlift) return;
  val[q] = A[slot[q]];
  A[slot[q]] = 0.0;
}

__global__ void k_bc_rows(int nbc, const int32_t* __restrict__ dofs, const int32_t* __restrict__ rowptr,
                          const int32_t* __restrict__ colidx, double* __restrict__ A) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nbc) return;
  const int row = dofs[q];
  for (int k = rowptr[row]; k < rowptr[row + 1]; ++k) A[k] = (colidx[k] == row) ? 1.0 : 0.0;
}

__global__ void k_dinv(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                       const double* __restrict__ A, double* __restrict__ dinv) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  double d = 0.0;
  for (int k = rowptr[row]; k < rowptr[row + 1]; ++k)
    if (colidx[k] == row) d = A[k];
  dinv[row] = 1.0 / d;
}

// b[row] -= sum_q lift_val[q] * g[lift_bc[q]]   (fixed order -> reproducible)
__global__ void k_lift(int nrows, const int32_t* __restrict__ rows, const int32_t* __restrict__ ptr,
                       const int32_t* __restrict__ bc, const double* __restrict__ val,
                       const double* __restrict__ g, double* __restrict__ b) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nrows) return;
  double s = 0.0;
  for (int k = ptr[q]; k < ptr[q + 1]; ++k) s += val[k] * g[bc[k]];
  b[rows[q]] -= s;
}

// set_bc on the right-hand side and on the PCG start vector (u_B = g)
__global__ void k_set_bc(int nbc, const int32_t* __restrict__ dofs, const double* __restrict__ g,
                         double* __restrict__ b, double* __restrict__ u) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nbc) return;
  b[dofs[q]] = g[q];
  u[dofs[q]] = g[q];
}

__global__ void k_gather(int ns, const int32_t* __restrict__ idx, const double* __restrict__ u,
                         double* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < ns) out[q] = u[idx[q]];
}

// Hold load of a pre-heated transient (hf_hold_load): F_i = (K u)_i on the rows outside the transient's Dirichlet set B
// (mask[i] = 0), F_i = 0 on B.  One lane per row, products summed in CSR order (bitwise reproducible); runs once per run.
__global__ __launch_bounds__(TPB) void k_hold_load(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                   const double* __restrict__ K, const double* __restrict__ u,
                                                   const unsigned char* __restrict__ mask, double* __restrict__ F) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  double s = 0.0;
  if (!mask[row])
    for (int k = rowptr[row]; k < rowptr[row + 1]; ++k) s += K[k] * u[colidx[k]];
  F[row] = s;
}

__global__ void k_mark_rows(int nq, const int32_t* __restrict__ idx, unsigned char* __restrict__ mask) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nq) mask[idx[q]] = 1;
}

// ------------------------------------------------------------------------------------------
// CSR SpMV, LDS-staged ("CSR-stream"): a workgroup takes chunks of RB consecutive rows; all
// 256 lanes stream the chunk's values and column indices in nnz order (fully coalesced) and
// park val*x[col] in LDS; then lane t sums the products of row t in column order.  The
// summation order per row is the CSR order -> bitwise reproducible, no atomics.
//   MODE 0: y = A x
//   MODE 2: r = b - A x; p = D^-1 r; partials r.p, p.p, (D^-1 b)^2   (PCG start)
//   MODE 3: y = b - A x                                              (multigrid residual)
//   MODE 4: y = x + w D^-1 (b - A x), partials b.y                   (damped-Jacobi sweep, fused r.z)
//   MODE 5: y = b - A x; p = w D^-1 y; partials (D^-1 y)^2, (D^-1 b)^2   (AMG-PCG start)
//   MODE 6: y += A x                                                 (multigrid prolongation)
//   MODE 7: y = A x, partials b.y                                    (fused up leg of the finest level: z = GP [r; e], r.z)
//   MODE 8: y = A x; p = 2 x - b        (RHS b = M u^n fused with the extrapolated start
//           2 u^n - u^{n-1} of the next solve; `b` carries u^{n-1})
//   MODE 9: PCG iteration head (x = z): convergence test, beta, Ap <- A z + beta Ap, p <- z + beta p,
//           p.Ap partials - SpMV and direction update in one pass
//   MODE 10: y = A x + w F            (RHS with a load: b = M u^n + dt F; F comes in the `dinv` operand)
//   MODE 11: y = A x + w F; p = 2 x - b   (MODE 8 with the load of MODE 10)
//   MODE 12..15: BDF2 right-hand sides, `b` carries u^{n-1} and the operand is formed while the column slice is staged:
//   MODE 12: y = A (4/3 x - 1/3 b); p = x             (p: the copy of u^n that becomes the next step's u^{n-1})
//   MODE 13: y = A (4/3 x - 1/3 b); p = 2 x - b       (with the extrapolated start vector, as MODE 8)
//   MODE 14: MODE 12 + w F    MODE 15: MODE 13 + w F  (load in the `dinv` operand, as MODE 10 / 11)
// The chunk is `rpc` rows (512 for the fine operator; fewer for long-row transfer operators so
// that a chunk's products fit the 64-KB LDS window).
// ------------------------------------------------------------------------------------------
// Compressed column indices of the fine operator (C16): per 512-row chunk the sorted list of the columns it
// touches (`dict`, ~1.3 entries per row: the chunk's own rows plus a halo) and a 16-bit position in that list
// per nonzero instead of the 32-bit column.  The chunk's slice of x is staged in LDS once (an almost contiguous
// gather) and the products look it up there: 10 instead of 12 bytes per nonzero, 5x fewer global gathers.
// progress of the solve for the host (ScalMirror): payload first, then the counter the host polls
__device__ __forceinline__ unsigned long long mirror_stamp(unsigned epoch, int v) {
  return (static_cast<unsigned long long>(epoch) << 32) | static_cast<unsigned>(v);
}
__device__ __forceinline__ void mirror_publish(ScalMirror* m, double zz, int iters, int done, unsigned epoch) {
  if (m == nullptr) return;
  m->zz = zz;
  m->iters = iters;
  __hip_atomic_store(&m->done_st, mirror_stamp(epoch, done), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();
  __hip_atomic_store(&m->tested_st, mirror_stamp(epoch, iters + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void mirror_breakdown(ScalMirror* m, unsigned epoch) {
  if (m != nullptr) __hip_atomic_store(&m->done_st, mirror_stamp(epoch, 2), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// own != 0 (square operators whose rows all store their diagonal): the chunk's own rows are a contiguous run of its sorted
// column list, so the row-wise operand x[row] of MODE 4 / 8 / 9 is taken from the staged slice instead of read again.
struct ColComp { const int32_t* dptr; const int32_t* dict; const uint16_t* id; int xd_off; int own; };
// Value lists of the fine operator (VC, with C16): per chunk the distinct 64-bit patterns of its values (`vlist`, starts in
// `vptr`, ascending as unsigned integers) and per nonzero one word cv = column position | value position << 16, instead of an
// f64 value and a 16-bit column position: 4 + 8 (list entries / nnz) instead of 10 bytes per nonzero, the same doubles
// multiplied.  Lists of up to `vcap` entries are staged in LDS behind the operand slice (vl_off), longer ones are read in place.
struct ValComp : ColComp { const int32_t* vptr; const double* vlist; const uint32_t* cv; int vl_off; int vcap; };

// The matrix stream (values, 16-bit positions) is read exactly once per launch: HF_NT_STREAM=1 marks those loads non-temporal
// (A/B builds; 0 = plain loads)
#ifndef HF_NT_STREAM
#define HF_NT_STREAM 0
#endif
#ifndef HF_PIPE
#define HF_PIPE 1      // chunk pipeline: 1 = single-precision operators (the transfer operators), 2 = all, 0 = none (A/B builds)
#endif
// HF_PHASE_CLOCK=<mode> (measurement builds only, scripts/phase_clock.py): lane 0 of every workgroup of k_spmv<mode, C16>
// stamps the 100 MHz clock at its phase boundaries (entry, then per chunk: operand slice staged, products parked, rows
// summed) into g_phase[workgroup][16]; hf_debug_phases copies the table out
#ifndef HF_PHASE_CLOCK
#define HF_PHASE_CLOCK -1
#endif
#if HF_PHASE_CLOCK >= 0
#ifndef HF_PHASE_CONV
#define HF_PHASE_CONV 0   // MODE 0 only: 1 = the launch that carries the convergence test (fused restriction of the finest level)
#endif
__device__ unsigned long long g_phase[MAXP * 16];
#define HF_STAMP(slot)                                                                                   \
  do {                                                                                                   \
    if (MODE == HF_PHASE_CLOCK && C16 && (MODE != 0 || (part2 != nullptr) == (HF_PHASE_CONV != 0)) && threadIdx.x == 0 && (slot) < 16) \
      g_phase[blockIdx.x * 16 + (slot)] = wall_clock64();                                                \
  } while (0)
#else
#define HF_STAMP(slot) do { } while (0)
#endif
template <typename T>
__device__ __forceinline__ T stream_load(const T* p) {
#if HF_NT_STREAM
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}

// BDF2 operand of the right-hand side: 4/3 u^n - 1/3 u^{n-1}
__device__ __forceinline__ double bdf2_operand(double un, double unm1) { return (4.0 * un - unm1) * (1.0 / 3.0); }

// Variable-step BDF2 (hf_set_step): the operand a u^n - b u^{n-1} with a = (1+w)^2 / (1+2w), b = w^2 / (1+2w) of the
// step ratio w.  The VB instances of k_spmv (modes 12-15 only) take a and b behind the column tables; every other instance has the
// argument list of before.  bdf2_operand_var (above, with k_picard_w_var) is the one expression of it, uncontracted: the same bits wherever it is formed.
template <class Base>
struct BdfVarComp : Base { double ca, cb; };
template <bool VC, bool VB>
struct SpmvComp {
  using base = typename std::conditional<VC, ValComp, ColComp>::type;
  using type = typename std::conditional<VB, BdfVarComp<base>, base>::type;
};

template <int MODE, bool C16 = false, typename VT = double, int UN = 8, bool VC = false, bool VB = false>
__global__ __launch_bounds__(TS) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_spmv(int n, int nchunks, int rpc /* rows per chunk, <= TS */,
                                              const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                              const VT* __restrict__ vals, const double* __restrict__ x,
                                              double* __restrict__ y, Scal* __restrict__ scal,
                                              double* __restrict__ part0, const double* __restrict__ bvec,
                                              const double* __restrict__ dinv, double* __restrict__ pvec,
                                              double* __restrict__ part1, double* __restrict__ part2, double w,
                                              int npart /* partial slots the consumers sum (>= gridDim.x) */,
                                              int parity, typename SpmvComp<VC, VB>::type comp) {
  extern __shared__ double sprod[];
  __shared__ double s4[TS / 64];
  __shared__ int s_own;
  constexpr bool BDF = MODE >= 12 && MODE <= 15;   // operand x[c] -> 4/3 x[c] - 1/3 bvec[c] (VB: a x[c] - b bvec[c])
  static_assert(!VB || BDF, "variable BDF2 coefficients: the right-hand side modes 12-15 only");
  // the operand slice as staged: x, or the BDF2 combination of x and bvec (two gathers per list entry, one slice in LDS)
  auto opnd = [&](int c) {   // position of the chunk's first row in its column list (ColComp::own)
    if constexpr (VB) return bdf2_operand_var(comp.ca, comp.cb, x[c], bvec[c]);
    else return BDF ? bdf2_operand(x[c], bvec[c]) : x[c];
  };
  // launches inside the PCG loop return at once after convergence; MODE 0 / 7 are also used outside it (right-hand
  // side, debug products), where the launcher passes no `scal`
  if ((MODE == 3 || MODE == 4 || MODE == 6 || MODE == 9) && scal->done) return;
  if ((MODE == 0 || MODE == 7) && scal != nullptr && scal->done) return;
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
  double beta = 0.0;
  bool first9 = false;
  if (MODE == 9) {
    first9 = scal->first != 0;
    // PCG iteration head: x = z (preconditioned residual).  Convergence test on the (D^-1 r)^2 partials
    // of the last update, beta = r.z(new)/r.z(old) from the two parity slots (part1), then in the row
    // loop  Ap <- A z + beta Ap,  p <- z + beta p  (direction update by recurrence) and p.Ap partials.
    if (!first9) {
      double v0 = 0.0, v1 = 0.0, v2 = 0.0;
      for (int k = threadIdx.x; k < npart; k += TS) {
        v0 += part1[parity * MAXP + k];
        v1 += part1[(parity ^ 1) * MAXP + k];
        v2 += part2[k];
      }
      const double rz_new = block_sum<TS / 64>(v0, s4);
      const double rz_old = block_sum<TS / 64>(v1, s4);
      const double zz = block_sum<TS / 64>(v2, s4);
      const bool conv = zz <= scal->tol2;
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        scal->zz = zz;
        if (conv) scal->done = 1;
      }
      if (conv) return;
      beta = rz_new / rz_old;
    }
  }
  // first kernel of a V-cycle inside the PCG loop: the update that precedes it left the (D^-1 r)^2 partials of the new
  // iterate - if that iterate has converged, the cycle (and every later launch of this burst) is skipped here instead of
  // after the cycle, by the next iteration head.  True: converged, the caller returns.
  auto cycle_gate = [&]() {
    if (!((MODE == 3 || MODE == 0) && part2 != nullptr)) return false;
    double v2 = 0.0;
    for (int k = threadIdx.x; k < npart; k += TS) v2 += part2[k];
    const double zz = block_sum<TS / 64>(v2, s4);
    const bool conv = zz <= scal->tol2;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (conv) { scal->zz = zz; scal->done = 1; }
      mirror_publish(scal->mirror, zz, scal->iters, conv ? 1 : 0, scal->epoch);
    }
    return conv;
  };
  constexpr bool PIPELINED = C16 && !VC && (HF_PIPE == 2 || (HF_PIPE == 1 && sizeof(VT) == 4));
  static_assert(!VC || (C16 && sizeof(VT) == 8), "value lists: the fine operator's f64 arrays on compressed columns");
  if (!PIPELINED && cycle_gate()) return;     // (the pipelined path requests its first chunk before it adds up the partials)
  const ChunkIter sched(nchunks);
  HF_STAMP(0);
  int stamp_at = 1;
  (void)stamp_at;
  // Chunks of fewer rows than threads (transfer operators with long rows, MODE 0 / 6 / 7 only): tpr = TS / rpc lanes
  // share a row's sum, so the row-sum phase uses every lane
  const int tpr = (MODE == 0 || MODE == 6 || MODE == 7) ? TS / rpc : 1;
  const int prel = static_cast<int>(threadIdx.x) / tpr;
  const int psub = static_cast<int>(threadIdx.x) % tpr;
  struct RowOps { double b, d, y, p, x; };
  // row-wise epilogue operands, requested early so that their latency hides under the chunk's stream.  Unconditional loads
  // at a clamped row: a load under a divergent branch makes the compiler's wait counters inexact - every later wait
  // would then cover all loads in flight, the prefetched ones of the next chunk included
  auto row_operands = [&](int prc, bool from_slice) {
    RowOps e{0.0, 0.0, 0.0, 0.0, 0.0};
    if (MODE == 2 || MODE == 3 || MODE == 4 || MODE == 5 || MODE == 7 || MODE == 8 || MODE == 11 || MODE == 13 || MODE == 15) e.b = bvec[prc];
    if (MODE == 2 || MODE == 4 || MODE == 5 || MODE == 10 || MODE == 11 || MODE == 14 || MODE == 15) e.d = dinv[prc];
    if (MODE == 6 || (MODE == 9 && !first9)) e.y = y[prc];
    if (MODE == 9 && !first9) e.p = pvec[prc];
    if ((MODE == 4 || MODE == 8 || MODE == 9 || MODE == 11) && !from_slice) e.x = x[prc];
    if (BDF) e.x = x[prc];     // the staged slice holds the combination, not u^n
    return e;
  };
  // the chunk's products are parked in sprod: row sums in CSR order and the mode's epilogue
  auto rows_phase = [&](bool pin, int prow, int pa, int pb, const RowOps& e) {
    if ((MODE == 0 || MODE == 6 || MODE == 7) && tpr > 1) {
      // tpr is a power of two <= 16 (rpc >= 32): the lanes of a row are neighbours inside one wavefront
      double s = 0.0;
      if (pin)
        for (int j = pa + psub; j < pb; j += tpr) s += sprod[j];
      for (int o = tpr >> 1; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
      if (pin && psub == 0) {
        y[prow] = (MODE == 6) ? e.y + s : s;
        if (MODE == 7) acc0 += e.b * s;
      }
    } else if (pin) {
      const int row = prow;
      double s = 0.0;
      for (int j = pa; j < pb; ++j) s += sprod[j];
      if (MODE == 0) {
        y[row] = s;
      } else if (MODE == 2) {
        const double ri = e.b - s;
        const double zi = e.d * ri;
        y[row] = ri;
        pvec[row] = zi;
        acc0 += ri * zi;
        acc1 += zi * zi;
        acc2 += (e.d * e.b) * (e.d * e.b);
      } else if (MODE == 3) {
        y[row] = e.b - s;
      } else if (MODE == 4) {
        const double yi = e.x + w * e.d * (e.b - s);
        y[row] = yi;
        acc0 += e.b * yi;
      } else if (MODE == 5) {
        const double ri = e.b - s;
        y[row] = ri;
        pvec[row] = w * e.d * ri;
        acc1 += (e.d * ri) * (e.d * ri);
        acc2 += (e.d * e.b) * (e.d * e.b);
      } else if (MODE == 7) {
        y[row] = s;
        acc0 += e.b * s;
      } else if (MODE == 6) {
        y[row] = e.y + s;
      } else if (MODE == 8) {
        y[row] = s;
        pvec[row] = 2.0 * e.x - e.b;
      } else if (MODE == 10) {
        y[row] = s + w * e.d;
      } else if (MODE == 11) {
        y[row] = s + w * e.d;
        pvec[row] = 2.0 * e.x - e.b;
      } else if (BDF) {
        y[row] = (MODE == 14 || MODE == 15) ? s + w * e.d : s;
        pvec[row] = (MODE == 13 || MODE == 15) ? 2.0 * e.x - e.b : e.x;
      } else {
        const double api = first9 ? s : s + beta * e.y;          // first iteration: p = z, Ap = A z
        const double pi = first9 ? e.x : e.x + beta * e.p;
        y[row] = api;
        pvec[row] = pi;
        acc0 += pi * api;
      }
    }
  };
  if (PIPELINED) {
    // Software pipeline over the workgroup's chunks.  A chunk needs, in dependent order: its bounds -> the head of its
    // column list and its matrix stream (values, 16-bit positions) -> the gathered operand slice.  While chunk c is
    // worked on, the bounds, the list head and the first UN * TS entries of the stream of chunk c+1 are already in flight
    // (registers), so c+1 starts with its operand gathers and finds its stream landed.  Every load of the pipeline is
    // unconditional (clamped or parked index) - see row_operands.
    struct Bounds { int k0, k1, d0, d1; };
    auto bounds = [&](int ch) {
      Bounds q;
      const int a0 = ch * rpc, a1 = min(n, a0 + rpc);
      q.k0 = rowptr[a0]; q.k1 = rowptr[a1];
      q.d0 = comp.dptr[ch]; q.d1 = comp.dptr[ch + 1];
      return q;
    };
    int lhead[HF_STAGE_U];        // list head of the chunk about to start
    double v[UN];                 // its first UN * TS stream entries
    int id[UN];
    auto heads = [&](const Bounds& q, bool live) {
      // !live (no further chunk; q = the current one): every wavefront re-reads the chunk's first 32 entries, results
      // unused.  The offset stays a per-lane value on purpose: with a uniform parked index the compiler turns the loads
      // into scalar ones behind a branch and waits for every load in flight there.
      const int dl = max(q.d1 - 1, 0), kl = max(q.k1 - 1, 0);   // a chunk of empty rows has an empty list
      const int t = static_cast<int>(threadIdx.x);
#pragma unroll
      for (int u = 0; u < HF_STAGE_U; ++u) lhead[u] = comp.dict[min(q.d0 + (live ? t + u * TS : (t & 31)), dl)];
      __builtin_amdgcn_sched_barrier(0);   // list head first: the next chunk's gathers wait for it and for nothing younger
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int kk = min(q.k0 + (live ? t + u * TS : (t & 31)), kl);
        v[u] = static_cast<double>(stream_load(&vals[kk]));
        id[u] = static_cast<int>(stream_load(&comp.id[kk]));
      }
    };
    double* xd = sprod + comp.xd_off;
    Bounds cur = bounds(min(sched.chunk, nchunks - 1));
    heads(cur, sched.chunk < sched.end);
    if (cycle_gate()) return;       // the first chunk's requests are out: the test's reduction runs under their latency
    for (int chunk = sched.chunk; chunk < sched.end; chunk += sched.step) {
      const bool more = chunk + sched.step < sched.end;
      const int r0 = chunk * rpc, r1 = min(n, r0 + rpc);
      const int k0 = cur.k0, k1 = cur.k1, d0 = cur.d0, nd = cur.d1 - cur.d0;
      const int prow = r0 + prel;
      const bool pin = prow < r1;
      const int prc = min(prow, r1 - 1);
      // (1) operand gathers of the list head, then the next chunk's bounds, this lane's row bounds and row operands
      int c0[HF_STAGE_U];
      double x0[HF_STAGE_U];
#pragma unroll
      for (int u = 0; u < HF_STAGE_U; ++u) { c0[u] = lhead[u]; x0[u] = opnd(c0[u]); }
      const Bounds nxt = bounds(more ? chunk + sched.step : chunk);
      const int pa = rowptr[prc] - k0, pb = rowptr[prc + 1] - k0;
      RowOps e = row_operands(prc, comp.own != 0);
      // (2) operand slice into LDS
#pragma unroll
      for (int u = 0; u < HF_STAGE_U; ++u) {
        const int i = static_cast<int>(threadIdx.x) + u * TS;
        if (i < nd) {
          xd[i] = x0[u];
          if ((MODE == 4 || MODE == 8 || MODE == 9 || MODE == 11) && c0[u] == r0) s_own = i;
        }
      }
      for (int i = threadIdx.x + HF_STAGE_U * TS; i < nd; i += HF_STAGE_U * TS) {   // lists longer than the head (rare)
        int c[HF_STAGE_U];
        double xv[HF_STAGE_U];
#pragma unroll
        for (int u = 0; u < HF_STAGE_U; ++u) c[u] = comp.dict[d0 + min(i + u * TS, nd - 1)];
#pragma unroll
        for (int u = 0; u < HF_STAGE_U; ++u) xv[u] = opnd(c[u]);
#pragma unroll
        for (int u = 0; u < HF_STAGE_U; ++u)
          if (i + u * TS < nd) {
            xd[i + u * TS] = xv[u];
            if ((MODE == 4 || MODE == 8 || MODE == 9 || MODE == 11) && c[u] == r0) s_own = i + u * TS;
          }
      }
      __syncthreads();
      HF_STAMP(stamp_at); ++stamp_at;
      if ((MODE == 4 || MODE == 8 || MODE == 9 || MODE == 11) && comp.own && pin) e.x = xd[s_own + (prow - r0)];
      // (3) products in stream order
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int kk = k0 + static_cast<int>(threadIdx.x) + u * TS;
        if (kk < k1) sprod[kk - k0] = v[u] * xd[id[u]];
      }
      for (int kb = k0 + UN * TS; kb < k1; kb += UN * TS) {     // chunks longer than UN * TS entries (rare)
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          const int kk = min(kb + static_cast<int>(threadIdx.x) + u * TS, k1 - 1);
          v[u] = static_cast<double>(stream_load(&vals[kk]));
          id[u] = static_cast<int>(stream_load(&comp.id[kk]));
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          const int kk = kb + static_cast<int>(threadIdx.x) + u * TS;
          if (kk < k1) sprod[kk - k0] = v[u] * xd[id[u]];
        }
      }
      // (4) the next chunk's list head and stream head go out; they land while the rows are summed and stored
      heads(nxt, more);
      __syncthreads();
      HF_STAMP(stamp_at); ++stamp_at;
      rows_phase(pin, prow, pa, pb, e);
      __syncthreads();
      HF_STAMP(stamp_at); ++stamp_at;
      cur = nxt;
    }
  } else {
  const ChunkIter& sched_ = sched;
  for (int chunk = sched_.chunk; chunk < sched_.end; chunk += sched_.step) {
    const int r0 = chunk * rpc;
    const int r1 = min(n, r0 + rpc);
    const int k0 = rowptr[r0];
    const int k1 = rowptr[r1];
    const int prow = r0 + prel;
    const bool pin = prow < r1;
    int pa = 0, pb = 0;
    if (pin) {
      pa = rowptr[prow] - k0;
      pb = rowptr[prow + 1] - k0;
    }
    RowOps e = row_operands(min(prow, r1 - 1), C16 && comp.own != 0);
    if constexpr (VC) {
      // as the C16 branch below, on the packed stream: the first batch of words and the chunk's value list are requested before
      // the operand slice is staged, so the three latencies overlap
      double* xd = sprod + comp.xd_off;
      double* vl = sprod + comp.vl_off;
      const int d0 = comp.dptr[chunk], nd = comp.dptr[chunk + 1] - d0;
      const int v0 = comp.vptr[chunk], nv = comp.vptr[chunk + 1] - v0;
      const bool vin = nv <= comp.vcap;          // the same for every lane: the list sits in LDS, or is read in place
      int k = k0 + threadIdx.x;
      std::uint32_t cw[HF_UNROLL];
#pragma unroll
      for (int u = 0; u < HF_UNROLL; ++u) cw[u] = (k + u * TS < k1) ? stream_load(&comp.cv[k + u * TS]) : 0u;
      double lv[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = static_cast<int>(threadIdx.x) + u * TS;
        lv[u] = (vin && i < nv) ? comp.vlist[v0 + i] : 0.0;
      }
      for (int i = threadIdx.x; i < nd; i += HF_STAGE_U * TS) {
        int c[HF_STAGE_U];
        double xv[HF_STAGE_U];
#pragma unroll
        for (int u = 0; u < HF_STAGE_U; ++u) c[u] = (i + u * TS < nd) ? comp.dict[d0 + i + u * TS] : 0;
#pragma unroll
        for (int u = 0; u < HF_STAGE_U; ++u) xv[u] = (i + u * TS < nd) ? opnd(c[u]) : 0.0;
#pragma unroll
        for (int u = 0; u < HF_STAGE_U; ++u)
          if (i + u * TS < nd) {
            xd[i + u * TS] = xv[u];
            if ((MODE == 4 || MODE == 8 || MODE == 9 || MODE == 11) && c[u] == r0) s_own = i + u * TS;
          }
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int i = static_cast<int>(threadIdx.x) + u * TS;
        if (vin && i < nv) vl[i] = lv[u];
      }
      if (vin)
        for (int i = threadIdx.x + 2 * TS; i < nv; i += TS) vl[i] = comp.vlist[v0 + i];   // lists longer than 2 TS (rare)
      __syncthreads();
      HF_STAMP(stamp_at); ++stamp_at;
      if ((MODE == 4 || MODE == 8 || MODE == 9 || MODE == 11) && comp.own && pin) e.x = xd[s_own + (prow - r0)];
      while (k < k1) {
        const int kn = k + HF_UNROLL * TS;
        std::uint32_t cn[HF_UNROLL];
#pragma unroll
        for (int u = 0; u < HF_UNROLL; ++u) cn[u] = (kn + u * TS < k1) ? stream_load(&comp.cv[kn + u * TS]) : 0u;
        if (vin) {
#pragma unroll
          for (int u = 0; u < HF_UNROLL; ++u)
            if (k + u * TS < k1) sprod[k - k0 + u * TS] = vl[cw[u] >> 16] * xd[cw[u] & 0xffffu];
        } else {
          double gv[HF_UNROLL];
#pragma unroll
          for (int u = 0; u < HF_UNROLL; ++u) gv[u] = (k + u * TS < k1) ? comp.vlist[v0 + static_cast<int>(cw[u] >> 16)] : 0.0;
#pragma unroll
          for (int u = 0; u < HF_UNROLL; ++u)
            if (k + u * TS < k1) sprod[k - k0 + u * TS] = gv[u] * xd[cw[u] & 0xffffu];
        }
#pragma unroll
        for (int u = 0; u < HF_UNROLL; ++u) cw[u] = cn[u];
        k = kn;
      }
    } else if (C16) {
      // first batch of values / 16-bit ids is requested before the operand slice is staged, so both latencies overlap
      double* xd = sprod + comp.xd_off;
      const int d0 = comp.dptr[chunk], nd = comp.dptr[chunk + 1] - d0;
      int k = k0 + threadIdx.x;
      double v[HF_UNROLL];
      int id[HF_UNROLL];
#pragma unroll
      for (int u = 0; u < HF_UNROLL; ++u) {
        const bool in = k + u * TS < k1;
        v[u] = in ? static_cast<double>(stream_load(&vals[k + u * TS])) : 0.0;
        id[u] = in ? static_cast<int>(stream_load(&comp.id[k + u * TS])) : 0;
      }
      // HF_STAGE_U entries of the column list per lane and pass (the fine operator's lists hold 1.3 TS entries, those of the
      // transfer operators up to 3.5 TS): the list loads go out together and the gathers after them - dependent round
      // trips per chunk: two instead of two per TS entries
      for (int i = threadIdx.x; i < nd; i += HF_STAGE_U * TS) {
        int c[HF_STAGE_U];
        double xv[HF_STAGE_U];
#pragma unroll
        for (int u = 0; u < HF_STAGE_U; ++u) c[u] = (i + u * TS < nd) ? comp.dict[d0 + i + u * TS] : 0;
#pragma unroll
        for (int u = 0; u < HF_STAGE_U; ++u) xv[u] = (i + u * TS < nd) ? opnd(c[u]) : 0.0;
#pragma unroll
        for (int u = 0; u < HF_STAGE_U; ++u)
          if (i + u * TS < nd) {
            xd[i + u * TS] = xv[u];
            if ((MODE == 4 || MODE == 8 || MODE == 9 || MODE == 11) && c[u] == r0) s_own = i + u * TS;
          }
      }
      __syncthreads();
      HF_STAMP(stamp_at); ++stamp_at;
      if ((MODE == 4 || MODE == 8 || MODE == 9 || MODE == 11) && comp.own && pin) e.x = xd[s_own + (prow - r0)];
      while (k < k1) {
        const int kn = k + HF_UNROLL * TS;
        double vn[HF_UNROLL];
        int idn[HF_UNROLL];
#pragma unroll
        for (int u = 0; u < HF_UNROLL; ++u) {
          const bool in = kn + u * TS < k1;
          vn[u] = in ? static_cast<double>(stream_load(&vals[kn + u * TS])) : 0.0;
          idn[u] = in ? static_cast<int>(stream_load(&comp.id[kn + u * TS])) : 0;
        }
#pragma unroll
        for (int u = 0; u < HF_UNROLL; ++u)
          if (k + u * TS < k1) sprod[k - k0 + u * TS] = v[u] * xd[id[u]];
#pragma unroll
        for (int u = 0; u < HF_UNROLL; ++u) { v[u] = vn[u]; id[u] = idn[u]; }
        k = kn;
      }
    } else {
      // products in nnz order: HF_UNROLL predicated value/index loads, then the gathers, in flight per lane
      for (int k = k0 + threadIdx.x; k < k1; k += HF_UNROLL * TS) {
        int c[HF_UNROLL];
        double v[HF_UNROLL], xv[HF_UNROLL];
#pragma unroll
        for (int u = 0; u < HF_UNROLL; ++u) {
          const bool in = k + u * TS < k1;
          c[u] = in ? colidx[k + u * TS] : 0;
          v[u] = in ? static_cast<double>(vals[k + u * TS]) : 0.0;
        }
#pragma unroll
        for (int u = 0; u < HF_UNROLL; ++u) xv[u] = (k + u * TS < k1) ? opnd(c[u]) : 0.0;
#pragma unroll
        for (int u = 0; u < HF_UNROLL; ++u)
          if (k + u * TS < k1) sprod[k - k0 + u * TS] = v[u] * xv[u];
      }
    }
    __syncthreads();
    HF_STAMP(stamp_at); ++stamp_at;
    rows_phase(pin, prow, pa, pb, e);
    __syncthreads();
    HF_STAMP(stamp_at); ++stamp_at;
  }
  }
  // consumers sum `npart` slots in a fixed order; this launch has fewer workgroups, the rest are zeros
  if (MODE == 2 || MODE == 7 || MODE == 9 || (MODE == 4 && part0 != nullptr)) {
    const double t0 = block_sum<TS / 64>(acc0, s4);
    if (threadIdx.x == 0) {
      part0[blockIdx.x] = t0;
      for (int q = blockIdx.x + gridDim.x; q < npart; q += gridDim.x) part0[q] = 0.0;
    }
  }
  if (MODE == 2 || MODE == 5) {
    const double t1 = block_sum<TS / 64>(acc1, s4);
    const double t2 = block_sum<TS / 64>(acc2, s4);
    if (threadIdx.x == 0) {
      part1[blockIdx.x] = t1;
      part2[blockIdx.x] = t2;
      for (int q = blockIdx.x + gridDim.x; q < npart; q += gridDim.x) { part1[q] = 0.0; part2[q] = 0.0; }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Builder of the value lists (ValComp), three launches on the context's stream:
//   k_vl_ids    one workgroup per chunk: the chunk's values as (64-bit pattern, origin) pairs in LDS, bitonic sort over the chunk
//               padded to a power of two, list heads flagged and counted, cv[k] = column position | rank of vals[k] << 16
//   k_vl_scan   one workgroup: list starts = exclusive sum of the chunks' counts; {sum, max} for the host
//   k_vl_lists  vlist[vptr[chunk] + rank] = vals[k]; lanes that hold the same pattern store the same 8 bytes
// Patterns are compared as unsigned integers (0.0 and -0.0 are two entries); the same values give the same tables.
// ------------------------------------------------------------------------------------------
constexpr int VL_MAX_CHUNK = 4096;   // nonzeros of the largest chunk the builder sorts (40 KiB of LDS)

// inclusive sum over the workgroup's NW wavefronts; `total`: the workgroup's sum
template <int NW>
__device__ __forceinline__ int block_scan_incl(int v, int* sw, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) sw[w] = v;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int q = 0; q < NW; ++q) {
    const int t = sw[q];
    if (q < w) before += t;
    total += t;
  }
  __syncthreads();
  return v + before;
}

__global__ __launch_bounds__(TS) void k_vl_ids(int n, int nchunks, int rpc, const int32_t* __restrict__ rowptr,
                                               const double* __restrict__ vals, const uint16_t* __restrict__ cid,
                                               std::uint32_t* __restrict__ cv, int32_t* __restrict__ count) {
  __shared__ unsigned long long skey[VL_MAX_CHUNK];
  __shared__ uint16_t sorg[VL_MAX_CHUNK];
  __shared__ int sw[TS / 64];
  const int tid = static_cast<int>(threadIdx.x);
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int r0 = chunk * rpc, r1 = min(n, r0 + rpc);
    const int k0 = rowptr[r0], m = min(rowptr[r1] - k0, VL_MAX_CHUNK);   // (the host builds no lists for a mesh with longer chunks)
    int np = 64;
    while (np < m) np <<= 1;
    for (int i = tid; i < np; i += TS) {
      skey[i] = i < m ? static_cast<unsigned long long>(__double_as_longlong(vals[k0 + i])) : ~0ull;
      sorg[i] = static_cast<uint16_t>(i);
    }
    __syncthreads();
    // ascending by (pattern, origin): the pads (origin >= m) end up behind every entry of the chunk, whatever its pattern
    for (int size = 2; size <= np; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = tid; t < (np >> 1); t += TS) {
          const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
          const bool up = (lo & size) == 0;
          const unsigned long long ka = skey[lo], kb = skey[hi];
          const uint16_t oa = sorg[lo], ob = sorg[hi];
          const bool gt = ka > kb || (ka == kb && oa > ob);
          if (gt == up) { skey[lo] = kb; skey[hi] = ka; sorg[lo] = ob; sorg[hi] = oa; }
        }
        __syncthreads();
      }
    // each lane ranks `per` consecutive sorted entries
    const int per = (np + TS - 1) / TS;
    const int i0 = tid * per;
    int heads = 0;
    for (int j = 0; j < per; ++j) {
      const int i = i0 + j;
      if (i < m && (i == 0 || skey[i] != skey[i - 1])) ++heads;
    }
    int total = 0;
    int run = block_scan_incl<TS / 64>(heads, sw, total) - heads;   // list heads before this lane's entries
    for (int j = 0; j < per; ++j) {
      const int i = i0 + j;
      if (i < m) {
        if (i == 0 || skey[i] != skey[i - 1]) ++run;
        const int k = k0 + sorg[i];
        cv[k] = static_cast<std::uint32_t>(cid[k]) | (static_cast<std::uint32_t>(run - 1) << 16);
      }
    }
    if (tid == 0) count[chunk] = total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(1024) void k_vl_scan(int nchunks, const int32_t* __restrict__ count, int32_t* __restrict__ vptr,
                                                  int32_t* __restrict__ info) {
  __shared__ int sw[16];
  __shared__ int smax[16];
  const int tid = static_cast<int>(threadIdx.x);
  int carry = 0, mx = 0;
  for (int base = 0; base < nchunks; base += 1024) {
    const int i = base + tid;
    const int v = i < nchunks ? count[i] : 0;
    mx = max(mx, v);
    int total = 0;
    const int incl = block_scan_incl<16>(v, sw, total);
    if (i < nchunks) vptr[i] = carry + incl - v;
    carry += total;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_down(mx, o, 64));
  if ((tid & 63) == 0) smax[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    for (int q = 1; q < 16; ++q) mx = max(mx, smax[q]);
    vptr[nchunks] = carry;
    info[0] = carry;
    info[1] = mx;
  }
}

__global__ __launch_bounds__(TS) void k_vl_lists(int n, int nchunks, int rpc, const int32_t* __restrict__ rowptr,
                                                 const double* __restrict__ vals, const std::uint32_t* __restrict__ cv,
                                                 const int32_t* __restrict__ vptr, long long cap, double* __restrict__ vlist) {
  if (vptr[nchunks] > cap) return;     // more list entries than the array holds: the host keeps the raw path
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int r0 = chunk * rpc, r1 = min(n, r0 + rpc);
    const int k0 = rowptr[r0], k1 = rowptr[r1], v0 = vptr[chunk];
    for (int k = k0 + threadIdx.x; k < k1; k += TS) vlist[v0 + static_cast<int>(cv[k] >> 16)] = vals[k];
  }
}

// PCG start: tolerance and convergence of the initial iterate (one workgroup).
__global__ __launch_bounds__(TPB) void k_pcg_begin(int P, double rtol, double atol, const double* __restrict__ part_zz,
                                                   const double* __restrict__ part_bn, Scal* __restrict__ scal, unsigned epoch) {
  __shared__ double s4[4];
  const double zz = sum_partials(part_zz, P, s4);
  const double bn2 = sum_partials(part_bn, P, s4);
  if (threadIdx.x == 0) {
    // relative to the right-hand side; a zero right-hand side (the exact answer is then zero) with a non-zero start vector
    // - a warm-started projection of a field that has gone flat - is measured against the start residual instead
    const double tol = fmax(rtol * sqrt(bn2 > 0.0 ? bn2 : zz), atol);
    scal->tol2 = tol * tol;
    scal->bn2 = bn2;
    scal->zz = zz;
    scal->iters = 0;
    scal->first = 1;
    scal->done = (zz <= tol * tol) ? 1 : 0;
    scal->epoch = epoch;
    if (scal->mirror != nullptr) scal->mirror->bn2 = bn2;
    mirror_publish(scal->mirror, zz, 0, scal->done, epoch);
  }
}

// x += alpha p; r -= alpha Ap; z = D^-1 r; partials r.z (into the other parity slot), z.z
__global__ __launch_bounds__(TPB) void k_pcg_update(int n, int nchunks, int P, int parity, Scal* __restrict__ scal,
                                                    const double* __restrict__ part_pAp, double* __restrict__ part_rz,
                                                    double* __restrict__ part_zz, double* __restrict__ x,
                                                    double* __restrict__ r, const double* __restrict__ p,
                                                    const double* __restrict__ Ap, const double* __restrict__ dinv,
                                                    double* __restrict__ z) {
  __shared__ double s4[4];
  if (scal->done) return;
  const double pAp = sum_partials(part_pAp, P, s4);
  const double rz = sum_partials(part_rz + parity * MAXP, P, s4);
  if (!(pAp > 0.0)) {                                   // breakdown (A_hat is SPD, so only on NaN/garbage)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      scal->done = 2;
      mirror_breakdown(scal->mirror, scal->epoch);
    }
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { scal->iters += 1; scal->first = 0; }
  const double alpha = rz / pAp;
  double a_rz = 0.0, a_zz = 0.0;
  const ChunkIter sched(nchunks);
  for (int chunk = sched.chunk; chunk < sched.end; chunk += sched.step) {
    const int i = chunk * RB + threadIdx.x;
    if (i < n) {
      const double ri = r[i] - alpha * Ap[i];
      const double zi = dinv[i] * ri;
      x[i] += alpha * p[i];
      r[i] = ri;
      z[i] = zi;
      a_rz += ri * zi;
      a_zz += zi * zi;
    }
  }
  const double t0 = block_sum(a_rz, s4);
  const double t1 = block_sum(a_zz, s4);
  if (threadIdx.x == 0) {
    part_rz[(parity ^ 1) * MAXP + blockIdx.x] = t0;
    part_zz[blockIdx.x] = t1;
  }
}

// ------------------------------------------------------------------------------------------
// Generic CSR SpMV for the multigrid transfer operators and coarse levels: LANES lanes of a
// wavefront share one row (4..64 by the average row length), four predicated loads + gathers in
// flight per lane (the fused legs have rows of hundreds of entries), fixed-order shuffle reduction.
//   VMODE 0: y = A x      1: y += A x
// ------------------------------------------------------------------------------------------
template <int LANES, int VMODE, typename VT = double>
__global__ __launch_bounds__(TPB) void k_spmv_vec(int nrow, const int32_t* __restrict__ ptr,
                                                  const int32_t* __restrict__ idx, const VT* __restrict__ val,
                                                  const double* __restrict__ x, double* __restrict__ y,
                                                  const Scal* __restrict__ scal) {
  if (scal->done) return;
  const int lane = threadIdx.x % LANES;
  const int rows_per_pass = (gridDim.x * TPB) / LANES;
  for (int row = (blockIdx.x * TPB + threadIdx.x) / LANES; row < nrow; row += rows_per_pass) {
    const int k1 = ptr[row + 1];
    const double y0 = (VMODE == 1 && lane == 0) ? y[row] : 0.0;
    double s = 0.0;
    for (int k = ptr[row] + lane; k < k1; k += 4 * LANES) {
      int c[4];
      double v[4], xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool in = k + u * LANES < k1;
        c[u] = in ? idx[k + u * LANES] : 0;
        v[u] = in ? static_cast<double>(val[k + u * LANES]) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) xv[u] = (k + u * LANES < k1) ? x[c[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < 4; ++u) s += v[u] * xv[u];
    }
#pragma unroll
    for (int o = LANES / 2; o > 0; o >>= 1) s += __shfl_down(s, o, LANES);
    if (lane == 0) y[row] = (VMODE == 1) ? y0 + s : s;
  }
}

// Same operation for operators with very long rows (the fused down leg onto a small level): a whole
// workgroup per row, four predicated loads + gathers in flight per lane, fixed-order block reduction.
template <int VMODE, typename VT = double>
__global__ __launch_bounds__(TPB) void k_spmv_row(int nrow, const int32_t* __restrict__ ptr,
                                                  const int32_t* __restrict__ idx, const VT* __restrict__ val,
                                                  const double* __restrict__ x, double* __restrict__ y,
                                                  const Scal* __restrict__ scal) {
  __shared__ double s4[TPB / 64];
  if (scal->done) return;
  for (int row = blockIdx.x; row < nrow; row += gridDim.x) {
    const int k1 = ptr[row + 1];
    const double y0 = (VMODE == 1 && threadIdx.x == 0) ? y[row] : 0.0;
    double s = 0.0;
    for (int k = ptr[row] + threadIdx.x; k < k1; k += 4 * TPB) {
      int c[4];
      double v[4], xv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const bool in = k + u * TPB < k1;
        c[u] = in ? idx[k + u * TPB] : 0;
        v[u] = in ? static_cast<double>(val[k + u * TPB]) : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) xv[u] = (k + u * TPB < k1) ? x[c[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < 4; ++u) s += v[u] * xv[u];
    }
    const double t = block_sum<TPB / 64>(s, s4);
    if (threadIdx.x == 0) y[row] = (VMODE == 1) ? y0 + t : t;
  }
}

// start vector: u = base + sum_k c_k w_k   (base = 2 u^n - u^{n-1}; w_k = boundary responses)
struct RespArgs { const double* w[MAXRESP]; double c[MAXRESP]; int k; };
__global__ __launch_bounds__(TPB) void k_start_vector(int n, const double* __restrict__ base, RespArgs a,
                                                      double* __restrict__ u) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    double s = base[i];
    for (int k = 0; k < a.k; ++k) s += a.c[k] * a.w[k][i];
    u[i] = s;
  }
}

// ------------------------------------------------------------------------------------------
// Start vector by Galerkin projection (hf_set_start_vector kind 3; Fischer 1998, "Projection techniques for
// iterative solution of Ax = b with successive right-hand sides").  The free part of each of the last few
// solutions u^k solves A_ff v = f^k with a known right-hand side, and so do the boundary responses w = R d.  The
// start vector of the next solve is the combination of those vectors that is closest to the new solution in the
// A-norm: G alpha = h with G_kl = V_k . F_l, h_k = V_k . f.  V_k holds u^k with its Dirichlet entries zeroed (so
// every dot product runs over the free rows only), F_k the right-hand side b^k as it was.
// ------------------------------------------------------------------------------------------
// (PROJ_MH solutions kept + MAXRESP boundary responses = PROJ_MT vectors: hf_context.hpp; HF_PROJ_MH for A/B builds)
struct ProjVecs { const double* V[PROJ_MT]; int slot[PROJ_MT]; int m; };

// partial sums of h_k = V_k . f and (Fnew != null) of the Gram column g_k = V_k . Fnew, one pass over all vectors
__global__ __launch_bounds__(TPB) void k_proj_dots(int n, ProjVecs a, const double* __restrict__ f, const double* __restrict__ Fnew,
                                                   double* __restrict__ part /* [2 * PROJ_MT][MAXP] */) {
  __shared__ double sw[TPB / 64][2 * PROJ_MT];
  double ah[PROJ_MT], ag[PROJ_MT];
#pragma unroll
  for (int k = 0; k < PROJ_MT; ++k) { ah[k] = 0.0; ag[k] = 0.0; }
  // two rows per pass: the loads of both (up to 2 m + 4) are in flight together - the stored vectors come from HBM
  const int stride = gridDim.x * TPB;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += 2 * stride) {
    const int i2 = i + stride;
    const bool two = i2 < n;
    const double fi = f ? f[i] : 0.0, gi = Fnew ? Fnew[i] : 0.0;
    const double fj = (f && two) ? f[i2] : 0.0, gj = (Fnew && two) ? Fnew[i2] : 0.0;
    double v0[PROJ_MT], v1[PROJ_MT];
#pragma unroll
    for (int k = 0; k < PROJ_MT; ++k) {
      v0[k] = k < a.m ? a.V[k][i] : 0.0;
      v1[k] = (k < a.m && two) ? a.V[k][i2] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < PROJ_MT; ++k) {
      ah[k] += v0[k] * fi;
      ag[k] += v0[k] * gi;
      ah[k] += v1[k] * fj;
      ag[k] += v1[k] * gj;
    }
  }
  // all 2m sums through one barrier: shuffle tree per wavefront, then the four wave sums in wave order (block_sum's order)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < PROJ_MT; ++k)
    if (k < a.m) {
      double th = ah[k], tg = ag[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { th += __shfl_down(th, o, 64); tg += __shfl_down(tg, o, 64); }
      if (lane == 0) { sw[wave][2 * k] = th; sw[wave][2 * k + 1] = tg; }
    }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < 2 * a.m) {
    double t = sw[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < TPB / 64; ++w) t += sw[w][threadIdx.x];
    part[threadIdx.x * MAXP + blockIdx.x] = t;
  }
}

// One workgroup: finish the sums (a wavefront per sum, fixed order), store the Gram column of slot `jnew` (if >= 0),
// and (do_solve) solve the scaled normal equations by symmetric elimination with diagonal pivoting (the matrix is
// positive semi-definite, so its largest remaining entry sits on the diagonal); directions whose pivot falls below
// 1e-12 of the first are left out (nearly dependent solutions).  alpha[slot] receives the coefficients (0 for
// slots left out), alpha[PROJ_MT] the rank.
static_assert(PROJ_MT * PROJ_MT <= 1024, "k_proj_solve holds one matrix entry per thread");
constexpr int PROJ_SOLVE_T = 1024;   // 16 wavefronts: one or two partial arrays each (the sums are the long part of the kernel)
__global__ __launch_bounds__(PROJ_SOLVE_T) void k_proj_solve(int P, ProjVecs a, int jnew, int do_solve, double* __restrict__ part,
                                                    double* __restrict__ G /* [PROJ_MT][PROJ_MT] by slot */, double* __restrict__ alpha) {
  __shared__ double sh[PROJ_MT], sg[PROJ_MT];
  __shared__ double A[PROJ_MT][PROJ_MT + 1], bb[PROJ_MT], dd[PROJ_MT], xx[PROJ_MT];
  __shared__ int perm[PROJ_MT], piv, stop, rank_s;
  __shared__ double pmax;
  // batched loop: one workgroup per column, each with its own partial sums, Gram matrix and coefficients
  part += static_cast<size_t>(blockIdx.x) * 2 * PROJ_MT * MAXP;
  G += blockIdx.x * PROJ_MT * PROJ_MT;
  alpha += blockIdx.x * (PROJ_MT + 1);
  const int m = a.m, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int q = wave; q < 2 * m; q += PROJ_SOLVE_T / 64) {  // sum q: partial array q of `part`
    double v = 0.0;
    for (int k0 = 0; k0 < P; k0 += 256) {
      double e[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const int k = k0 + lane + 64 * u; e[u] = k < P ? part[q * MAXP + k] : 0.0; }
      v += (e[0] + e[1]) + (e[2] + e[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) { if (q & 1) sg[q >> 1] = v; else sh[q >> 1] = v; }
  }
  __syncthreads();
  if (jnew >= 0 && t < m) { G[a.slot[t] * PROJ_MT + jnew] = sg[t]; G[jnew * PROJ_MT + a.slot[t]] = sg[t]; }
  if (!do_solve) return;
  __syncthreads();                                          // the column just written is read below (same workgroup)
  if (t < PROJ_MT + 1) alpha[t] = 0.0;
  if (t < m) {
    double gii = (jnew >= 0 && a.slot[t] == jnew) ? sg[t] : G[a.slot[t] * PROJ_MT + a.slot[t]];
    const bool ok = gii > 0.0 && gii < 1e300;
    dd[t] = ok ? 1.0 / sqrt(gii) : 0.0;
    perm[t] = t;
    xx[t] = 0.0;
  }
  __syncthreads();
  const int i = t / PROJ_MT, j = t % PROJ_MT;
  if (i < m && j < m) {
    // entries of the new column come from shared memory (global writes of this launch are not re-read)
    double gij;
    if (jnew >= 0 && a.slot[j] == jnew) gij = sg[i];
    else if (jnew >= 0 && a.slot[i] == jnew) gij = sg[j];
    else gij = G[a.slot[i] * PROJ_MT + a.slot[j]];
    const bool ok = dd[i] > 0.0 && dd[j] > 0.0;
    A[i][j] = ok ? gij * dd[i] * dd[j] : (i == j ? 0.0 : 0.0);
  }
  if (t < m) bb[t] = sh[t] * dd[t];
  if (t == 0) { rank_s = 0; stop = 0; }
  __syncthreads();
  for (int c = 0; c < m; ++c) {
    if (t == 0) {
      int pi = c;
      double best = A[c][c];
      for (int q = c + 1; q < m; ++q)
        if (A[q][q] > best) { best = A[q][q]; pi = q; }
      if (c == 0) pmax = best;
      piv = pi;
      stop = !(best > 1e-12 * pmax) || !(best > 0.0);
    }
    __syncthreads();
    if (stop) break;
    const int pv = piv;
    if (pv != c) {                                          // symmetric interchange c <-> pv
      if (t < m) { const double x0 = A[c][t]; A[c][t] = A[pv][t]; A[pv][t] = x0; }
      __syncthreads();
      if (t < m) { const double x0 = A[t][c]; A[t][c] = A[t][pv]; A[t][pv] = x0; }
      if (t == 0) {
        const double x0 = bb[c]; bb[c] = bb[pv]; bb[pv] = x0;
        const int p0 = perm[c]; perm[c] = perm[pv]; perm[pv] = p0;
      }
      __syncthreads();
    }
    if (i > c && i < m && j > c && j < m) A[i][j] -= A[i][c] / A[c][c] * A[c][j];
    if (i > c && i < m && j == c) bb[i] -= A[i][c] / A[c][c] * bb[c];
    if (t == 0) rank_s = c + 1;
    __syncthreads();
  }
  if (t != 0) return;
  const int rank = rank_s;
  for (int c = rank - 1; c >= 0; --c) {
    double v = bb[c];
    for (int q = c + 1; q < rank; ++q) v -= A[c][q] * xx[q];
    xx[c] = v / A[c][c];
  }
  bool finite = true;
  for (int c = 0; c < rank; ++c) finite = finite && (fabs(xx[c]) < 1e300);
  if (!finite) return;                      // alpha = 0: the start vector falls back to the boundary values alone
  for (int c = 0; c < rank; ++c) alpha[a.slot[perm[c]]] = xx[c] * dd[perm[c]];
  alpha[PROJ_MT] = static_cast<double>(rank);
}

// u = sum_k alpha[slot_k] V_k   (Dirichlet entries come out zero: set_bc writes them afterwards)
__global__ __launch_bounds__(TPB) void k_proj_combine(int n, ProjVecs a, const double* __restrict__ alpha, double* __restrict__ u) {
  double c[PROJ_MT];
#pragma unroll
  for (int k = 0; k < PROJ_MT; ++k) c[k] = k < a.m ? alpha[a.slot[k]] : 0.0;
  const int stride = gridDim.x * TPB;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += 2 * stride) {      // two rows per pass, as k_proj_dots
    const int i2 = i + stride;
    const bool two = i2 < n;
    double v0[PROJ_MT], v1[PROJ_MT];
#pragma unroll
    for (int k = 0; k < PROJ_MT; ++k) {
      v0[k] = k < a.m ? a.V[k][i] : 0.0;
      v1[k] = (k < a.m && two) ? a.V[k][i2] : 0.0;
    }
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k < PROJ_MT; ++k) { s0 += c[k] * v0[k]; s1 += c[k] * v1[k]; }
    u[i] = s0;
    if (two) u[i2] = s1;
  }
}

// two vector copies in one launch (projection ring: solution and right-hand side)
__global__ __launch_bounds__(TPB) void k_copy2(int n, const double* __restrict__ a, double* __restrict__ a_out,
                                               const double* __restrict__ b, double* __restrict__ b_out) {
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) {
    a_out[i] = a[i];
    b_out[i] = b[i];
  }
}

__global__ void k_zero_entries(int nq, const int32_t* __restrict__ idx, double* __restrict__ v) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nq) v[idx[q]] = 0.0;
}

// Streaming read of two arrays with 16-byte loads (HF_K_STREAM_READ: the bandwidth ceiling SpMV is measured against)
__global__ __launch_bounds__(TS) void k_stream_read(size_t n16a, const double2* __restrict__ a, size_t n16b,
                                                    const double2* __restrict__ b, double* __restrict__ sink) {
  double s = 0.0;
  const size_t stride = static_cast<size_t>(gridDim.x) * TS;
  for (int pass = 0; pass < 2; ++pass) {
    const double2* __restrict__ p = pass ? b : a;
    const size_t n16 = pass ? n16b : n16a;
    size_t i = static_cast<size_t>(blockIdx.x) * TS + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) {
      const double2 v0 = p[i], v1 = p[i + stride], v2 = p[i + 2 * stride], v3 = p[i + 3 * stride];
      s += (v0.x + v0.y) + (v1.x + v1.y) + (v2.x + v2.y) + (v3.x + v3.y);
    }
    for (; i < n16; i += stride) { const double2 v = p[i]; s += v.x + v.y; }
  }
  if (s == 1.2345678e301) sink[0] = s;   // never true for real data; keeps the loads alive
}

// x = w D^-1 b  (first damped-Jacobi sweep from a zero guess)
__global__ __launch_bounds__(TPB) void k_scale(int n, double w, const double* __restrict__ dinv,
                                               const double* __restrict__ b, double* __restrict__ x,
                                               const Scal* __restrict__ scal) {
  if (scal->done) return;
  for (int i = blockIdx.x * TPB + threadIdx.x; i < n; i += gridDim.x * TPB) x[i] = w * dinv[i] * b[i];
}

// x = Ainv b with the dense inverse of the coarsest operator (row-major, leading dimension ld, even):
// two wavefronts per row, 16-byte loads, halves combined through LDS.
__global__ __launch_bounds__(TPB) void k_dense_mv(int n, int ld, const double* __restrict__ Ainv,
                                                  const double* __restrict__ b, double* __restrict__ x,
                                                  const Scal* __restrict__ scal) {
  __shared__ double half_sum[4];
  if (scal->done) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;            // 0..3: waves 0,1 -> row 2*blk, waves 2,3 -> row 2*blk + 1
  const int npair = (n + 1) >> 1;
  for (int pr = blockIdx.x; pr < npair; pr += gridDim.x) {
    const int row = 2 * pr + (wave >> 1);
    double s = 0.0;
    if (row < n) {
      const double2* arow = reinterpret_cast<const double2*>(Ainv + static_cast<size_t>(row) * ld);
      const double2* bv = reinterpret_cast<const double2*>(b);
      const int nv = ld >> 1;
      for (int j = (wave & 1) * 64 + lane; j < nv; j += 128) {
        const double2 a = arow[j];
        const double2 v = bv[j];
        s += a.x * v.x + a.y * v.y;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) half_sum[wave] = s;
    __syncthreads();
    if (lane == 0 && (wave & 1) == 0 && row < n) x[row] = half_sum[wave] + half_sum[wave + 1];
    __syncthreads();
  }
}

// The same with the inverse stored in float (the preconditioner's operators are kept in single precision, the
// vectors and every accumulation stay double): 16-byte loads of four entries.
__global__ __launch_bounds__(TPB) void k_dense_mv_f32(int n, int ld /* multiple of 4 */, const float* __restrict__ Ainv,
                                                      const double* __restrict__ b, double* __restrict__ x,
                                                      const Scal* __restrict__ scal) {
  __shared__ double half_sum[4];
  if (scal->done) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int npair = (n + 1) >> 1;
  for (int pr = blockIdx.x; pr < npair; pr += gridDim.x) {
    const int row = 2 * pr + (wave >> 1);
    double s = 0.0;
    if (row < n) {
      const float4* arow = reinterpret_cast<const float4*>(Ainv + static_cast<size_t>(row) * ld);
      const double2* bv = reinterpret_cast<const double2*>(b);
      const int nv = ld >> 2;
      for (int j = (wave & 1) * 64 + lane; j < nv; j += 128) {
        const float4 a = arow[j];
        const double2 v0 = bv[2 * j], v1 = bv[2 * j + 1];
        s += static_cast<double>(a.x) * v0.x + static_cast<double>(a.y) * v0.y + static_cast<double>(a.z) * v1.x + static_cast<double>(a.w) * v1.y;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) half_sum[wave] = s;
    __syncthreads();
    if (lane == 0 && (wave & 1) == 0 && row < n) x[row] = half_sum[wave] + half_sum[wave + 1];
    __syncthreads();
  }
}

__global__ void k_to_float(size_t n, const double* __restrict__ src, float* __restrict__ dst) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * blockDim.x)
    dst[i] = static_cast<float>(src[i]);
}

// Dense inverse of the coarsest operator on the GPU: blocked Gauss-Jordan without pivoting (the operator is SPD, its pivots
// stay positive).  W = [A | I] (n x 2n, row pitch 2n) is reduced to [I | A^-1], GJ_B pivots per step.  At the step of pivot block
// [c0, c0 + b) only the n columns [c0 + b, n + c0 + b) can still change (those to the left of the block are finished unit columns
// and never read again, those to the right of the window still hold the identity's zeros), so a step is
//   k_gjb_rows:   R = D^-1 W(block rows, window), D = W(block, block) inverted in LDS by every workgroup for itself
//   k_gjb_update: W(i, window) -= W(i, block) R for the rows outside the block, W(block rows, window) = R
// - n^2 entries read and written per GJ_B pivots instead of 2 n^2 per pivot (1634 rows: 85 MB per pivot before, 30 ms in all).
constexpr int GJ_B = 32;
__global__ __launch_bounds__(TPB) void k_gjb_rows(int n, int c0, int b, const double* __restrict__ W, double* __restrict__ R /* [GJ_B][n] */) {
  __shared__ double D[GJ_B][GJ_B + 1], Di[GJ_B][GJ_B + 1];
  const int t = threadIdx.x, ld = 2 * n;
  for (int q = t; q < GJ_B * GJ_B; q += TPB) {
    const int r = q / GJ_B, c = q % GJ_B;
    D[r][c] = (r < b && c < b) ? W[static_cast<size_t>(c0 + r) * ld + c0 + c] : (r == c ? 1.0 : 0.0);
    Di[r][c] = r == c ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int p = 0; p < b; ++p) {                    // Gauss-Jordan on [D | Di], one pivot per round
    const double piv = D[p][p];
    __syncthreads();
    for (int q = t; q < 2 * GJ_B; q += TPB) {
      if (q < GJ_B) D[p][q] /= piv; else Di[p][q - GJ_B] /= piv;
    }
    __syncthreads();
    for (int q = t; q < GJ_B * 2 * GJ_B; q += TPB) {
      const int r = q / (2 * GJ_B), c = q % (2 * GJ_B);
      if (r == p) continue;
      const double f = D[r][p];
      if (c < GJ_B) { if (c != p) D[r][c] -= f * D[p][c]; } else Di[r][c - GJ_B] -= f * Di[p][c - GJ_B];
    }
    __syncthreads();
    for (int r = t; r < GJ_B; r += TPB)
      if (r != p) D[r][p] = 0.0;
    __syncthreads();
  }
  // this workgroup's columns of the window
  for (int j = blockIdx.x * TPB + t; j < n; j += gridDim.x * TPB) {
    const size_t col = static_cast<size_t>(c0 + b + j);
    double w[GJ_B];
#pragma unroll
    for (int r = 0; r < GJ_B; ++r) w[r] = r < b ? W[static_cast<size_t>(c0 + r) * ld + col] : 0.0;
    for (int r = 0; r < b; ++r) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < GJ_B; ++c) s += Di[r][c] * w[c];
      R[static_cast<size_t>(r) * n + j] = s;
    }
  }
}

// W = [A | I] from the coarsest operator in CSR form (W zeroed before): a thread per row
__global__ void k_gjb_fill(int n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx, const double* __restrict__ val,
                           double* __restrict__ W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double* w = W + static_cast<size_t>(i) * 2 * n;
  for (int k = ptr[i]; k < ptr[i + 1]; ++k) w[idx[k]] = val[k];
  w[n + i] = 1.0;
}

// 64 x 64 tile of the window per workgroup, 4 x 4 entries per thread; the tile's slices of the pivot columns and of R in LDS
__global__ __launch_bounds__(TPB) void k_gjb_update(int n, int c0, int b, double* __restrict__ W, const double* __restrict__ R) {
  __shared__ double sC[64][GJ_B + 1], sR[GJ_B][64 + 1];
  const int ld = 2 * n, t = threadIdx.x;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  for (int q = t; q < 64 * GJ_B; q += TPB) {
    const int r = q / GJ_B, c = q % GJ_B;
    sC[r][c] = (i0 + r < n && c < b) ? W[static_cast<size_t>(i0 + r) * ld + c0 + c] : 0.0;
  }
  for (int q = t; q < GJ_B * 64; q += TPB) {
    const int r = q / 64, c = q % 64;
    sR[r][c] = (r < b && j0 + c < n) ? R[static_cast<size_t>(r) * n + j0 + c] : 0.0;
  }
  __syncthreads();
  const int ti = (t / 16) * 4, tj = (t % 16) * 4;
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
  for (int k = 0; k < GJ_B; ++k) {
    double cu[4], rv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) cu[u] = sC[ti + u][k];
#pragma unroll
    for (int v = 0; v < 4; ++v) rv[v] = sR[k][tj + v];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] += cu[u] * rv[v];
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + ti + u;
    if (i >= n) continue;
    const bool pivot_row = i >= c0 && i < c0 + b;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + tj + v;
      if (j >= n) continue;
      double* w = W + static_cast<size_t>(i) * ld + c0 + b + j;
      *w = pivot_row ? sR[i - c0][tj + v] : *w - acc[u][v];
    }
  }
}

// AMG-PCG: x += alpha p; r -= alpha Ap; z0 = w D^-1 r (pre-smoothed start of the V-cycle);
// partial (D^-1 r)^2 for the convergence test.  r.z comes from the V-cycle's last kernel.
__global__ __launch_bounds__(TPB) void k_pcg_update_amg(int n, int nchunks, int P, int parity, Scal* __restrict__ scal,
                                                        const double* __restrict__ part_pAp,
                                                        const double* __restrict__ part_rz, double* __restrict__ part_zz,
                                                        double* __restrict__ x, double* __restrict__ r,
                                                        const double* __restrict__ p, const double* __restrict__ Ap,
                                                        const double* __restrict__ dinv, double w, double* __restrict__ z0) {
  __shared__ double s4[4];
  if (scal->done) return;
  const double pAp = sum_partials(part_pAp, P, s4);
  const double rz = sum_partials(part_rz + parity * MAXP, P, s4);
  if (!(pAp > 0.0)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      scal->done = 2;
      mirror_breakdown(scal->mirror, scal->epoch);
    }
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) { scal->iters += 1; scal->first = 0; }
  const double alpha = rz / pAp;
  double a_zz = 0.0;
  const ChunkIter sched(nchunks);
  for (int chunk = sched.chunk; chunk < sched.end; chunk += sched.step) {
    const int i = chunk * RB + threadIdx.x;
    if (i < n) {
      const double ri = r[i] - alpha * Ap[i];
      const double zi = dinv[i] * ri;
      x[i] += alpha * p[i];
      r[i] = ri;
      if (z0 != nullptr) z0[i] = w * zi;      // not needed when the finest level runs through its fused legs
      a_zz += zi * zi;
    }
  }
  const double t1 = block_sum(a_zz, s4);
  if (threadIdx.x == 0) part_zz[blockIdx.x] = t1;
}

}  // namespace
