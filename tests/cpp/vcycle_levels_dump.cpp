// Writes a multigrid hierarchy built by heatflow_amd/csrc/amg_host.hpp as raw arrays, for the float64 restatements of
// the V-cycle (tests/vcycle_oracle.py, run by tests/test_vcycle_oracle_cpu.py).  Model operator: 5-point Laplacian plus
// mass with a coefficient jump and one eliminated (unit) row, as in amg_host_check.cpp.
//   vcycle_levels_dump NX NY FUSE0 OUT      FUSE0: 0 explicit finest level, 1 both legs fused, 2 fused down leg only
// OUT: int32 nl, fine operator A0; per level: int32 n, f64 omega, f64 dinv[n], then A (level 0: empty), P, R, Rt, GP,
// each as int32 nrow, ncol, nnz, ptr[nrow + 1], idx[nnz], f64 val[nnz] (nrow = 0: absent).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "amg_host.hpp"

using amg::Csr;

static void put_csr(std::FILE* f, const Csr& m) {
  const int32_t hdr[3] = {m.nrow, m.ncol, static_cast<int32_t>(m.idx.size())};
  std::fwrite(hdr, sizeof(int32_t), 3, f);
  if (m.nrow == 0) return;
  std::fwrite(m.ptr.data(), sizeof(int32_t), m.ptr.size(), f);
  std::fwrite(m.idx.data(), sizeof(int32_t), m.idx.size(), f);
  std::fwrite(m.val.data(), sizeof(double), m.val.size(), f);
}

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: %s NX NY FUSE0 OUT\n", argv[0]); return 2; }
  const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]), fuse0 = std::atoi(argv[3]);
  const int n = nx * ny;
  Csr A;
  A.nrow = A.ncol = n;
  A.ptr.assign(n + 1, 0);
  auto kx_right = [&](int i) { return (i + 1 < nx / 2) ? 1.0 : 40.0; };   // coupling (i, i+1): the right cell's coefficient
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) {
      const int r = j * nx + i;
      if (r == 7) { A.idx.push_back(r); A.val.push_back(1.0); A.ptr[r + 1] = static_cast<int>(A.idx.size()); continue; }
      auto add = [&](int c, double v) { if (c != 7) { A.idx.push_back(c); A.val.push_back(v); } };
      const double kl = i > 0 ? kx_right(i - 1) : 0.0;
      double diag = 0.3 + (j > 0 ? 1.0 : 0.0) + (j < ny - 1 ? 1.0 : 0.0) + kl + (i < nx - 1 ? kx_right(i) : 0.0);
      if (j > 0) add(r - nx, -1.0);
      if (i > 0) add(r - 1, -kl);
      add(r, diag);
      if (i < nx - 1) add(r + 1, -kx_right(i));
      if (j < ny - 1) add(r + nx, -1.0);
      A.ptr[r + 1] = static_cast<int>(A.idx.size());
    }
  const Csr A0 = A;
  amg::Hierarchy H;
  amg::Params prm;
  prm.coarse_size = 40;
  prm.fuse_fine = fuse0 != 0;
  prm.fuse_fine_down_only = fuse0 == 2;
  if (!amg::build(std::move(A), prm, H)) { std::fprintf(stderr, "build failed\n"); return 1; }
  std::FILE* f = std::fopen(argv[4], "wb");
  if (!f) return 1;
  const int32_t nl = static_cast<int32_t>(H.levels.size());
  std::fwrite(&nl, sizeof nl, 1, f);
  put_csr(f, A0);
  for (const amg::Level& L : H.levels) {
    const int32_t ln = static_cast<int32_t>(L.dinv.size());
    std::fwrite(&ln, sizeof ln, 1, f);
    std::fwrite(&L.omega, sizeof(double), 1, f);
    std::fwrite(L.dinv.data(), sizeof(double), L.dinv.size(), f);
    put_csr(f, L.A); put_csr(f, L.P); put_csr(f, L.R); put_csr(f, L.Rt); put_csr(f, L.GP);
  }
  std::fclose(f);
  std::printf("levels %d\n", nl);
  return 0;
}
