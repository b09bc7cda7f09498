"""Float64 / longdouble restatement of the read-flux projection (hf_flux_setup, hf_flux_solve / hf_flux_project / hf_flux_sample,
the flux arguments of hf_batch_run_flux; k_grad_rows, k_grad_rhs, batch_flux_step).  TEST CODE: plain numpy / scipy, no device,
written from the algebra, not from the kernels' loops.

The projection g_c (c = z, r) of grad T onto P1 with weight r solves  M1 g_c = b_c,  M1_ab = int phi_a phi_b r dx,
    b_c[i] = sum over the triangles e at node i of (d_c T)_e w_{e,i},     w_{e,i} = |K_e| (2 r_i + r_j + r_k) / 12 = int_e phi_i r dx.
Per triangle (i, j, k):  d = (z_j - z_i)(r_k - r_i) - (z_k - z_i)(r_j - r_i),  |K| = |d| / 2,
    (d_z T)_e = (u_i (r_j - r_k) + u_j (r_k - r_i) + u_k (r_i - r_j)) / d,   (d_r T)_e = (u_i (z_k - z_j) + u_j (z_i - z_k) + u_k (z_j - z_i)) / d.
The magnitude sums a bound on b scales with:  S_c[i] = sum_e w_{e,i} (|u_i beta_i| + |u_j beta_j| + |u_k beta_k|) / |d|, beta the
coefficients above.  b cancels against S by up to 1e7 (a smooth field on a 300 K offset), so bounds are relative to S, never to |b|.

Evaluations (rhs): "ld" - everything in np.longdouble, rounded once at the end; float64: "asc" - per row, the row's node as vertex i
of every triangle, triangles in ascending order; "desc" - descending; "swap" - ascending with j and k exchanged (d and both
numerators change sign, their roundings change); "bincount" - the gradient once per triangle in its stored vertex order, np.bincount
(the shape of oracle.heat_oracle.GradientProjector).  Their differences are the restatement's own rounding spread.

The solves are pcg_oracle's loop as it stands (Column, pcg, pcg_batch: matrix M1, Jacobi, atol 0, x0 = the previous projection of
that component, zero after hf_flux_setup): solve_variants / sequence below only feed it.

MUTATIONS names the faults tests/test_flux_oracle_cpu.py injects so that every bound has a floor under it."""
import numpy as np
import scipy.sparse as sp

import pcg_oracle as po

LD = np.longdouble
VARIANTS = ("asc", "desc", "swap", "bincount")
MUTATIONS = ("weight_plain_mean", "no_fabs", "components_exchanged", "state_of_next_column", "node_major_output", "warm_start_of_z")
ROW_TOL = 1e-13            # |b_dev - b_ld| <= ROW_TOL S per row: the figure the project's load kernels are held to
SELF_TOL = 1e-15           # every float64 evaluation of the restatement against the longdouble one, in units of S


# ----------------------------------------------------------------------------------------------------------------------
# meshes and states
# ----------------------------------------------------------------------------------------------------------------------
def jittered_lattice(nz, nr, flipped=False):
    """The jittered lattice of tests/test_gpu_dir_tangent.py; ``flipped``: every other triangle's vertex order reversed (d < 0)."""
    from test_gpu_dir_tangent import _jittered_lattice

    coords, tris = _jittered_lattice(nz, nr)
    if flipped:
        tris = tris.copy()
        tris[1::2] = tris[1::2][:, [0, 2, 1]]
    return coords, tris


def with_fan(coords, tris, nfan=32):
    """The mesh with a closed fan of ``nfan`` triangles appended as a separate component: its centre's row has nfan + 1 entries
    (beyond the row-gather lists' 32), every other triangle of the fan clockwise."""
    n0 = len(coords)
    ang = 2 * np.pi * np.arange(nfan) / nfan
    c = np.array([3.0e-6, 1.0e-6])
    rad = 0.4e-6 * (1.0 + 0.2 * np.cos(3 * ang))
    pts = np.vstack([c[None, :], c[None, :] + rad[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])])
    fan = np.array([[n0, n0 + 1 + q, n0 + 1 + (q + 1) % nfan] for q in range(nfan)], dtype=np.int32)
    fan[1::2] = fan[1::2][:, [0, 2, 1]]
    return np.vstack([coords, pts]), np.vstack([tris, fan]).astype(np.int32)


LIN = (300.0, 2.0e7, -3.1e7)          # a, c_z, c_r of the linear field T = a + c_z (z - z_min) + c_r r   (K, K/m)


def linear_field(coords, coef=LIN):
    z, r = coords[:, 0], coords[:, 1]
    return coef[0] + coef[1] * (z - z.min()) + coef[2] * r


def rough_field(coords, seed=11):
    """The sine-plus-noise field of test_gpu_dir_tangent.test_block_stride_loop_and_partial_last_block."""
    rng = np.random.default_rng(seed)
    return 300.0 + 50.0 * np.sin(3.0e6 * coords[:, 0] + 1.0) * np.cos(1.0e6 * coords[:, 1]) + rng.uniform(-1.0, 1.0, len(coords))


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
class FluxOracle:
    def __init__(self, coords, tris):
        self.coords = np.asarray(coords, dtype=np.float64)
        self.tris = np.asarray(tris, dtype=np.int64)
        self.n, self.ne = len(self.coords), len(self.tris)
        self.flat = self.tris.ravel()                                       # (triangle, vertex) pairs in triangle order
        pat = sp.coo_matrix((np.ones(9 * self.ne), (np.repeat(self.tris, 3, axis=1).ravel(), np.tile(self.tris, (1, 3)).ravel())),
                            shape=(self.n, self.n)).tocsr()
        pat.sum_duplicates()
        pat.sort_indices()
        self.rowptr, self.colidx = pat.indptr.astype(np.int32), pat.indices.astype(np.int32)
        self._mass = None

    # -- per triangle ----------------------------------------------------------------------------------------------
    def triangles(self, u, dtype=LD, order=(0, 1, 2), mutation=None):
        """Per triangle in the vertex order ``order`` (a permutation of the stored one): dict(d, gz, gr (ne,), w (ne, 3), az, ar
        (ne,): the magnitude sums of the numerators over |d|)."""
        p = self.coords[self.tris[:, list(order)]].astype(dtype)
        ue = np.asarray(u, dtype=np.float64)[self.tris[:, list(order)]].astype(dtype)
        z, r = p[:, :, 0], p[:, :, 1]
        d = (z[:, 1] - z[:, 0]) * (r[:, 2] - r[:, 0]) - (z[:, 2] - z[:, 0]) * (r[:, 1] - r[:, 0])
        bz = [r[:, 1] - r[:, 2], r[:, 2] - r[:, 0], r[:, 0] - r[:, 1]]
        br = [z[:, 2] - z[:, 1], z[:, 0] - z[:, 2], z[:, 1] - z[:, 0]]
        tz = [ue[:, a] * bz[a] for a in range(3)]
        tr = [ue[:, a] * br[a] for a in range(3)]
        gz, gr = ((tz[0] + tz[1]) + tz[2]) / d, ((tr[0] + tr[1]) + tr[2]) / d
        area = (d if mutation == "no_fabs" else np.abs(d)) / 2
        rs = (r[:, 0] + r[:, 1]) + r[:, 2]
        if mutation == "weight_plain_mean":
            w = np.stack([area * rs / 9] * 3, axis=1)
        else:
            w = np.stack([area * (r[:, a] + rs) / 12 for a in range(3)], axis=1)
        if mutation == "components_exchanged":
            gz, gr = gr, gz
        az = ((np.abs(tz[0]) + np.abs(tz[1])) + np.abs(tz[2])) / np.abs(d)
        ar = ((np.abs(tr[0]) + np.abs(tr[1])) + np.abs(tr[2])) / np.abs(d)
        return {"d": d, "gz": gz, "gr": gr, "w": w, "az": az, "ar": ar}

    # -- per row ---------------------------------------------------------------------------------------------------
    def _rowwise(self, u, dtype, swap, mutation):
        """(cz, cr, sz, sr): per (triangle, vertex) pair, in self.flat's order, the contribution to that vertex's row, formed with
        the row's node as vertex i of the triangle (then j, k in the stored cyclic order, or exchanged)."""
        cz, cr, sz, sr = (np.empty((self.ne, 3), dtype=dtype) for _ in range(4))
        for a in range(3):
            order = (a, (a + 2) % 3, (a + 1) % 3) if swap else (a, (a + 1) % 3, (a + 2) % 3)
            t = self.triangles(u, dtype, order, mutation)
            cz[:, a], cr[:, a] = t["gz"] * t["w"][:, 0], t["gr"] * t["w"][:, 0]
            sz[:, a], sr[:, a] = t["az"] * np.abs(t["w"][:, 0]), t["ar"] * np.abs(t["w"][:, 0])
        return cz.ravel(), cr.ravel(), sz.ravel(), sr.ravel()

    def _sum(self, c, reverse=False):
        out = np.zeros(self.n, dtype=c.dtype)
        if reverse:
            np.add.at(out, self.flat[::-1], c[::-1])           # ufunc.at adds one entry after the other, in the order given
        else:
            np.add.at(out, self.flat, c)
        return out

    def rhs(self, u, variant="ld", mutation=None):
        """(b_z, b_r, S_z, S_r) as float64 vectors."""
        if variant == "bincount":
            t = self.triangles(u, np.float64, mutation=mutation)
            bz = np.bincount(self.flat, weights=(t["gz"][:, None] * t["w"]).ravel(), minlength=self.n)
            br = np.bincount(self.flat, weights=(t["gr"][:, None] * t["w"]).ravel(), minlength=self.n)
            sz = np.bincount(self.flat, weights=(t["az"][:, None] * np.abs(t["w"])).ravel(), minlength=self.n)
            sr = np.bincount(self.flat, weights=(t["ar"][:, None] * np.abs(t["w"])).ravel(), minlength=self.n)
            return bz, br, sz, sr
        dtype = LD if variant == "ld" else np.float64
        cz, cr, sz, sr = self._rowwise(u, dtype, variant == "swap", mutation)
        rev = variant == "desc"
        return tuple(self._sum(c, rev).astype(np.float64) for c in (cz, cr, sz, sr))

    # -- M1, D^-1 --------------------------------------------------------------------------------------------------
    def mass(self):
        """(M1 as a float64 csr_matrix on (rowptr, colidx), D^-1), summed in longdouble and rounded once:
        M_aa = |K| (6 r_a + 2 r_b + 2 r_c) / 60,  M_ab = |K| (2 r_a + 2 r_b + r_c) / 60."""
        if self._mass is None:
            p = self.coords[self.tris].astype(LD)
            z, r = p[:, :, 0], p[:, :, 1]
            area = np.abs((z[:, 1] - z[:, 0]) * (r[:, 2] - r[:, 0]) - (z[:, 2] - z[:, 0]) * (r[:, 1] - r[:, 0])) / 2
            rs = r.sum(axis=1)
            rows_of = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.rowptr))
            keys = rows_of * self.n + self.colidx
            data = np.zeros(len(self.colidx), dtype=LD)
            for a in range(3):
                for b in range(3):
                    val = area * 2 * (rs + 2 * r[:, a]) / 60 if a == b else area * (rs + r[:, a] + r[:, b]) / 60
                    slot = np.searchsorted(keys, self.tris[:, a] * self.n + self.tris[:, b])
                    np.add.at(data, slot, val)
            M = sp.csr_matrix((data.astype(np.float64), self.colidx, self.rowptr), shape=(self.n, self.n))
            self._mass = (M, 1.0 / M.diagonal())
        return self._mass

    def spectrum(self):
        """(lambda_min, lambda_max) of D^-1 M1, from the symmetric D^-1/2 M1 D^-1/2 (eigsh; the smallest by shift-invert at 0)."""
        import scipy.sparse.linalg as spla

        M, dinv = self.mass()
        s = sp.diags(np.sqrt(dinv))
        S = (s @ M @ s).tocsc()
        hi = spla.eigsh(S, k=1, which="LA", return_eigenvectors=False, tol=1e-8)[0]
        lo = spla.eigsh(S, k=1, sigma=0.0, which="LM", return_eigenvectors=False, tol=1e-8)[0]
        return float(lo), float(hi)


def row_ratio(got, ref, S):
    """max_i |got - ref|_i / S_i (a row with S = 0 must agree exactly)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(S > 0, np.abs(got - ref) / S, np.where(got == ref, 0.0, np.inf))
    return float(q.max())


# ----------------------------------------------------------------------------------------------------------------------
# the solves: pcg_oracle's loop on (M1, Jacobi)
# ----------------------------------------------------------------------------------------------------------------------
def solve(M, dinv, b, x0, rtol, sums="ld", max_it=5000):
    return po.pcg(M, b, x0, po.jacobi(dinv), dinv, rtol, 0.0, max_it=max_it, sums=sums)


def solve_variants(M, dinv, b, x0, rtol, max_it=5000):
    """(longdouble run, [the float64 variants' runs, cut at its count]) - the six evaluations of pcg_oracle.VARIANTS."""
    rl = solve(M, dinv, b, x0, rtol, max_it=max_it)
    return rl, [solve(M, dinv, b, x0, rtol, sums=v, max_it=max(rl["count"], 1)) for v in po.VARIANTS[1:]]


def solve_batch(M, dinv, bs, x0s, rtol, sums="ld", max_it=5000):
    """The nv columns stepped together (pcg_oracle.pcg_batch): per column its result; the device reports max over the counts."""
    cols = [po.Column(M, b, x0, po.jacobi(dinv), dinv, rtol, 0.0, sums) for b, x0 in zip(bs, x0s)]
    return po.pcg_batch(cols, max_it=max_it)


def final(res):
    return res["x"][res["count"]]


def sequence(M, dinv, rhs_steps, rtol, mutation=None, sums="ld"):
    """Consecutive projections of both components, each warm-started from its own previous projection (zero at first).
    rhs_steps: [(b_z, b_r)].  warm_start_of_z: the r solve starts from the z projection just solved, and the next z solve from the last
    r projection (the exchange of the two stored projections left out).  Returns [(res_z, res_r)]."""
    n = M.shape[0]
    gz, gr, out = np.zeros(n), np.zeros(n), []
    for bz, br in rhs_steps:
        rz = solve(M, dinv, bz, gz, rtol, sums)
        gz = final(rz)
        if mutation == "warm_start_of_z":
            rr = solve(M, dinv, br, gz, rtol, sums)
            gz = final(rr)                                # one stored vector serves both: the next z solve starts from this
        else:
            rr = solve(M, dinv, br, gr, rtol, sums)
            gr = final(rr)
        out.append((rz, rr))
    return out
