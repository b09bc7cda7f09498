"""How redundant the values of the GPU-assembled fine operators are, per 512-row SpMV chunk:
python scripts/value_share.py [mesh scale ...]      (default: 1.0 = stock mesh, 0.43 = C3)

For A = M + dt K (after the Dirichlet elimination) and M as hf_get_csr downloads them: distinct 64-bit patterns per chunk
(mean / median / p90 / max), their sum over the chunks relative to nnz - the share of a value id's list in the stream of
k_spmv's value-list path, (4 + 8 share) bytes per nonzero - and the share of chunks whose list fits a cap of 512 / 640 / 768 /
1024 entries.  The diagonals are counted on their own as well (they are sums of ~6 visits in list order)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import build_case          # noqa: E402
from helpers import make_problem        # noqa: E402

RPC = 512


def chunk_stats(rowptr, colidx, vals):
    n = len(rowptr) - 1
    bits = vals.view(np.uint64)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    isdiag = colidx == rows
    counts, dcounts, sizes = [], [], []
    for r0 in range(0, n, RPC):
        k0, k1 = rowptr[r0], rowptr[min(n, r0 + RPC)]
        counts.append(len(np.unique(bits[k0:k1])))
        dcounts.append(len(np.unique(bits[k0:k1][isdiag[k0:k1]])))
        sizes.append(k1 - k0)
    return np.array(counts), np.array(dcounts), np.array(sizes)


def main():
    scales = [float(a) for a in sys.argv[1:]] or [1.0, 0.43]
    for scale in scales:
        cfg, stack, mesh = build_case("geballe_with_diamond", scale)
        prob = make_problem(cfg, stack, mesh)
        try:
            rowptr, colidx, A, M = prob.backend.get_csr(values=True)
        finally:
            prob.close()
        nnz = len(colidx)
        for name, v in (("A", A), ("M", M)):
            c, d, s = chunk_stats(rowptr, colidx, v)
            caps = " ".join(f"<={cap}: {100.0 * np.mean(c <= cap):.1f}%" for cap in (512, 640, 768, 1024))
            print(f"scale {scale} n {len(rowptr) - 1} nnz {nnz} {name}: distinct per chunk mean {c.mean():.0f} median {np.median(c):.0f} "
                  f"p90 {np.percentile(c, 90):.0f} max {c.max()} | sum/nnz {c.sum() / nnz:.4f} | diagonals mean {d.mean():.0f} max {d.max()} | "
                  f"largest chunk {s.max()} nnz | chunks within cap {caps}", flush=True)


if __name__ == "__main__":
    main()
