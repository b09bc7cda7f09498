"""Float64 / longdouble restatement of the two PCG loops (pcg_solve in hf_solver.hpp with k_pcg_begin, k_pcg_update,
k_pcg_update_amg and the iteration heads of k_spmv; BatchOps::pcg_run in hf_batch.hpp with kb_begin, kb_update, kb_reduce).
TEST CODE: plain numpy / scipy, no device.  One restatement serves both loops: a batch is nv independent columns, each with
its own operator, stepped together, where a converged column stops changing.

The recurrences, statement for statement as the device forms them (x, r, p, Ap, z are float64 vectors):

    start     r = b - A x0;  zd = D^-1 r;  zz = zd.zd;  bn2 = (D^-1 b).(D^-1 b);  tol = max(rtol sqrt(bn2), atol)
              converged at once when zz <= tol^2;  z = B r;  rz = r.z
    head k    beta = rz / rz_old (k > 0);  Ap <- A z + beta Ap;  p <- z + beta p;  pAp = p.Ap      (Ap by recurrence, not A p)
    update k  alpha = rz / pAp;  r <- r - alpha Ap;  x <- x + alpha p;  zd = D^-1 r;  zz = zd.zd;  count += 1
    test      zz <= tol^2 ends the solve: the iterate is tested before its cycle (the multigrid loop tests in the first kernel
              of the cycle, the Jacobi loop in the next iteration head - the same iterate, the same quantity, the same outcome)
    cycle     z = B r;  rz_old = rz;  rz = r.z

Jacobi: B r = D^-1 r (= zd).  Multigrid: B = vcycle_oracle.stored_cycle on the parsed hierarchy; its z0 = w D^-1 r is the cycle's
pre-smoothed start, not the tested quantity.  The reported residual is sqrt(zz / bn2).

Variants (Variant, VARIANTS): "ld" takes every dot product, sum of partials and row of A v in np.longdouble and rounds each vector
statement y + a x once (the vectors stay float64); "chunk" multiplies in float64, sums each 256-row chunk in float64 and then the
chunk sums in float64 - the shape of the device's partials - and rounds y + a x twice; the others change the chunk size, sum
pairwise, or sum the rows of A v in longdouble under float64 dot products.  Their differences are the restatement's own rounding
spread, from which the bounds of tests/test_gpu_pcg_loops.py are taken (10 x).

MUTATIONS names the faults that tests/test_pcg_oracle_cpu.py injects so that every bound has a floor under it."""
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import vcycle_oracle as vo

LD = np.longdouble
RB = 256            # rows per chunk of the update kernels (hf_context.hpp)
ATOL_FACTOR = 1e3   # the GPU tests' deciding absolute tolerance: ATOL_FACTOR x rtol x |D^-1 b|
BAND = 1.01         # a count is asserted only when no tested residual lies within [tol / BAND, BAND tol]

MUTATIONS = ("beta_parity", "alpha_stale", "test_on_r", "tol_on_start", "test_late", "no_post_smoothing",
             "batch_frozen_updates", "batch_alpha_of_next")


# ----------------------------------------------------------------------------------------------------------------------
# sums
# ----------------------------------------------------------------------------------------------------------------------
# One way of evaluating the statements.  sums: "ld" - every dot product, row sum and y + a x in longdouble, rounded once; "chunk" -
# float64 products summed in chunks of chunk_rows rows and then over the chunks; "pairwise" - float64 products under numpy's
# pairwise summation.  ld_rows: the rows of A v are summed in longdouble (always under "ld"; an option under float64 sums).
Variant = namedtuple("Variant", "sums chunk_rows ld_rows", defaults=(0, False))
LD_VARIANT, CHUNK = Variant("ld", 0, True), Variant("chunk", 256)           # CHUNK: the shape of the device's partials
# the family of evaluations the spread is taken over
VARIANTS = (LD_VARIANT, CHUNK, Variant("chunk", 64), Variant("chunk", 1024), Variant("pairwise"), Variant("chunk", 256, ld_rows=True))
# float64 evaluations outside the family: they play the device in tests/test_pcg_oracle_cpu.py
OUTSIDE = (Variant("chunk", 512), Variant("chunk", 100))
_BY_NAME = {"ld": LD_VARIANT, "chunk": CHUNK}


def dot(a, b, sums=LD_VARIANT):
    v = _BY_NAME.get(sums, sums)
    if v.sums == "ld":
        return np.dot(a.astype(LD), b.astype(LD))
    prod = a * b
    if v.sums == "pairwise":
        return float(np.sum(prod))
    part = np.add.reduceat(prod, np.arange(0, len(prod), v.chunk_rows))
    s = 0.0
    for t in part:
        s += float(t)
    return s


def grid_shape(n):
    """(chunks, P): 256-row chunks and the workgroups of an update kernel launch."""
    chunks = -(-n // RB)
    P = min(chunks, 1024)
    if P >= 64:
        P &= ~7
    return chunks, P


# ----------------------------------------------------------------------------------------------------------------------
# preconditioners
# ----------------------------------------------------------------------------------------------------------------------
def jacobi(dinv):
    return lambda r: dinv * r


def multigrid(H, A0, dinv0, explicit=False):
    """The stored cycle of hierarchy H; ``explicit``: the finest level the way the batched cycle runs it."""
    return lambda r: vo.stored_cycle(H, A0, dinv0, r, explicit=explicit)


def cycle_without_post_smoothing(H, A0, dinv0):
    """The explicit cycle with its last sweep left out: B is no longer symmetric (mutation no_post_smoothing)."""
    return lambda r: vo.stored_cycle(H, A0, dinv0, r, explicit=True, post=False)


# ----------------------------------------------------------------------------------------------------------------------
# the loop
# ----------------------------------------------------------------------------------------------------------------------
class Column:
    """One PCG column, advanced statement by statement.  After begin(): done, tol, bn2.  x_k, alpha_k, beta_k, zz_k are kept."""

    def __init__(self, A, b, x0, B, dinv, rtol, atol=0.0, sums="ld", mutation=None):
        sums = _BY_NAME.get(sums, sums)
        self.A, self.b, self.B, self.dinv, self.sums, self.mut = sp.csr_matrix(A), np.asarray(b, dtype=np.float64), B, dinv, sums, mutation
        self.ld = sums.sums == "ld"
        self.ld_rows = sums.ld_rows
        if self.ld_rows:
            self.A.sort_indices()
            self.A_ld = self.A.data.astype(LD)
            self.rows = np.flatnonzero(np.diff(self.A.indptr))
        x = np.array(x0, dtype=np.float64)
        r = (self.b.astype(LD) - self._matvec(x, rounded=False)).astype(np.float64) if self.ld_rows else self.b - A @ x
        zd = dinv * r
        db = dinv * self.b
        on_r = mutation == "test_on_r"
        zz = self._dot(r, r) if on_r else self._dot(zd, zd)
        bn2 = self._dot(self.b, self.b) if on_r else self._dot(db, db)
        base = zz if (mutation == "tol_on_start" or not bn2 > 0) else bn2
        self.tol = max(float(rtol * np.sqrt(base)), float(atol))
        self.tol2 = self.tol * self.tol
        self.bn2 = float(bn2)
        self.x, self.r = x, r
        self.p = self.Ap = None
        self.xs, self.alphas, self.betas, self.zzs = [x.copy()], [], [], [float(zz)]
        self.count = 0
        self.done = self._converged()
        if not self.done:
            self.z = B(r)
            self.rz_hist = [self._dot(r, self.z)]

    def _dot(self, a, b):
        return dot(a, b, self.sums)

    def _matvec(self, v, rounded=True):
        """A v.  ld_rows: products and row sums in longdouble, rounded once (the device's kernels fuse the multiply-adds
        of a row; where b - A x0 cancels, as in a column that starts next to its solution, the roundings inside A x0 are what
        the iterates inherit); the other variants: scipy's float64 product."""
        if not self.ld_rows:
            return self.A @ v
        out = np.zeros(self.A.shape[0], dtype=LD)
        out[self.rows] = np.add.reduceat(self.A_ld * v[self.A.indices].astype(LD), self.A.indptr[self.rows])
        return out.astype(np.float64) if rounded else out

    def _axpy(self, y, a, x):
        """y + a x, stored in float64.  "ld": formed in longdouble and rounded once, which is what a fused multiply-add gives (the
        device's compiler contracts these statements); "chunk": two float64 roundings.  Both are valid float64 evaluations of
        the statement, so their difference belongs to the restatement's spread."""
        if self.ld:
            return (np.asarray(y).astype(LD) + LD(a) * x.astype(LD)).astype(np.float64)
        return np.asarray(y, dtype=np.float64) + a * x

    def _converged(self):
        if self.mut == "test_late":                  # the outcome of the iterate before this one
            return len(self.zzs) >= 2 and self.zzs[-2] <= self.tol2
        return self.zzs[-1] <= self.tol2

    def head(self):
        """beta, p, Ap, p.Ap; returns this iteration's alpha."""
        k = self.count
        rz = self.rz_hist[-1]
        if k == 0:
            self.p, self.Ap = self.z.copy(), self._matvec(self.z)
            self.betas.append(0.0)
        else:
            rz_old = self.rz_hist[max(len(self.rz_hist) - 3, 0)] if self.mut == "beta_parity" else self.rz_hist[-2]
            beta = float(rz / rz_old)
            self.Ap = self._axpy(self._matvec(self.z, rounded=not self.ld), beta, self.Ap)
            self.p = self._axpy(self.z, beta, self.p)
            self.betas.append(beta)
        pAp = self._dot(self.p, self.Ap)
        if self.mut == "alpha_stale" and k > 0:
            rz = self.rz_hist[-2]
        return float(rz / pAp)

    def update(self, alpha, record=True):
        self.r = self._axpy(self.r, -alpha, self.Ap)
        self.x = self._axpy(self.x, alpha, self.p)
        zd = self.dinv * self.r
        zz = self._dot(self.r, self.r) if self.mut == "test_on_r" else self._dot(zd, zd)
        self.zzs.append(float(zz))
        self.alphas.append(alpha)
        self.xs.append(self.x.copy())
        if record:
            self.count += 1
        self.done = self._converged()

    def cycle(self):
        self.z = self.B(self.r)
        self.rz_hist.append(self._dot(self.r, self.z))

    def result(self):
        n = self.count
        return {"x": self.xs, "alpha": self.alphas, "beta": self.betas, "zz": self.zzs, "count": n, "tol": self.tol,
                "bn2": self.bn2, "ratio": [float(np.sqrt(z)) / self.tol if self.tol > 0 else np.inf for z in self.zzs],
                "resid": float(np.sqrt(self.zzs[n] / max(self.bn2, 1e-300))), "converged": self.done}


def pcg(A, b, x0, B, dinv, rtol, atol=0.0, max_it=20000, sums="ld", mutation=None):
    """Every x_k (x[0] = x0), alpha_k, beta_k, the tested zz_k = |D^-1 r_k|^2, the count (number of updates), tol, per iterate
    its ratio sqrt(zz_k) / tol, the reported residual sqrt(zz_count / bn2) and whether the loop ended converged."""
    c = Column(A, b, x0, B, dinv, rtol, atol, sums, mutation)
    while not c.done and c.count < max_it:
        c.update(c.head())
        if not c.done:
            c.cycle()
    return c.result()


def pcg_batch(columns, max_it=20000, mutation=None):
    """``columns``: Column objects (begun).  Steps them together as the batched loop does; returns per column its result with
    "x" extended to every joint iteration (a frozen column repeats its last iterate) and "steps" = joint iterations run.
    batch_frozen_updates: a converged column goes on updating (its count stays); batch_alpha_of_next: column j steps with the
    alpha of column j + 1 (the last column with its own)."""
    nv = len(columns)
    frozen = [c.done for c in columns]
    traj = [[c.x.copy()] for c in columns]
    steps = 0
    while not all(frozen) and steps < max_it:
        live = [j for j in range(nv) if not frozen[j] or (mutation == "batch_frozen_updates" and columns[j].p is not None)]
        alphas = {j: columns[j].head() for j in live}
        for j in live:
            a = alphas[j]
            if mutation == "batch_alpha_of_next" and j + 1 in alphas:
                a = alphas[j + 1]
            columns[j].update(a, record=not frozen[j])
            if not frozen[j] and columns[j].done:
                frozen[j] = True
            if not columns[j].done or mutation == "batch_frozen_updates":
                columns[j].cycle()
        steps += 1
        for j in range(nv):
            traj[j].append(columns[j].x.copy())
    out = []
    for j, c in enumerate(columns):
        res = c.result()
        res["x"] = traj[j]
        res["steps"] = steps
        out.append(res)
    return out


def near_cut(res, upto=None):
    """The iterates (up to the count) whose tested residual lies within the band around tol: a count that hangs on one of them
    cannot be asserted as an equality."""
    upto = res["count"] if upto is None else upto
    return [k for k in range(upto + 1) if 1.0 / BAND <= res["ratio"][k] <= BAND]


# ----------------------------------------------------------------------------------------------------------------------
# metrics: functions of a list of iterates and (A, b)
# ----------------------------------------------------------------------------------------------------------------------
class Judge:
    """Holds (A, b, D^-1), the direct solution x* (scipy splu) and the scale |x* - x0|_inf of one linear system."""

    def __init__(self, A, b, dinv, x0, lu=None):
        """``lu``: the factorisation of an earlier Judge on the same A (Judge.lu), to be used again."""
        import scipy.sparse.linalg as spla

        self.A, self.b, self.dinv = sp.csr_matrix(A), np.asarray(b, dtype=np.float64), dinv
        self.lu = spla.splu(sp.csc_matrix(A)) if lu is None else lu
        self.xstar = self.lu.solve(self.b)
        self.scale = float(np.abs(self.xstar - x0).max())

    def _anorm(self, e):
        return float(np.sqrt(max(np.dot(e.astype(LD), (self.A @ e).astype(LD)), 0)))

    def iterate_error(self, xs, ref):
        """[|x_k - ref_k|_inf / |x* - x_0|_inf]"""
        s = self.scale if self.scale > 0 else 1.0
        return np.array([float(np.abs(x - y).max()) / s for x, y in zip(xs, ref)])

    def line_search(self, xs):
        """[|d_k . (b - A x_{k+1})| / (|d_k| |b - A x_{k+1}|)], d_k = x_{k+1} - x_k: zero for a correct alpha."""
        out = []
        for k in range(len(xs) - 1):
            d = xs[k + 1] - xs[k]
            r = self.b - self.A @ xs[k + 1]
            den = float(np.linalg.norm(d) * np.linalg.norm(r))
            out.append(abs(float(np.dot(d.astype(LD), r.astype(LD)))) / den if den > 0 else 0.0)
        return np.array(out)

    def conjugacy(self, xs):
        """(next[k] = |d_{k-1} . A d_k| / (|d_{k-1}|_A |d_k|_A): judges beta; far[k] = the largest over j < k - 1: judges the
        symmetry of B).  Entries for k >= 1 (far: k >= 2)."""
        d = [xs[k + 1] - xs[k] for k in range(len(xs) - 1)]
        Ad = [self.A @ v for v in d]
        nrm = [float(np.sqrt(max(np.dot(v.astype(LD), w.astype(LD)), 0))) for v, w in zip(d, Ad)]
        nxt, far = [], []
        for k in range(1, len(d)):
            vals = [abs(float(np.dot(d[j].astype(LD), Ad[k].astype(LD)))) / (nrm[j] * nrm[k]) if nrm[j] * nrm[k] > 0 else 0.0
                    for j in range(k)]
            nxt.append(vals[-1])
            far.append(max(vals[:-1]) if k >= 2 else 0.0)
        return np.array(nxt), np.array(far)

    def energy(self, xs):
        """[|x* - x_k|_A]: non-increasing."""
        return np.array([self._anorm(self.xstar - x) for x in xs])

    def energy_rise(self, xs):
        """The largest rise of the energy from one iterate to the next, relative to the start's energy (<= 0: none)."""
        e = self.energy(xs)
        return float(np.max(np.diff(e)) / e[0]) if len(e) > 1 and e[0] > 0 else 0.0

    def true_residual(self, x):
        """|D^-1 (b - A x)| / |D^-1 b|"""
        r = self.dinv * (self.b - self.A @ x)
        db = self.dinv * self.b
        return float(np.sqrt(np.dot(r.astype(LD), r.astype(LD)) / np.dot(db.astype(LD), db.astype(LD))))

    def residual_gap(self, x, reported, rtol):
        return abs(self.true_residual(x) - reported) / rtol

    def all(self, xs, ref=None):
        """{"iterate_error", "line_search", "conj_next", "conj_far": arrays by iterate; "energy_rise": a number}"""
        nxt, far = self.conjugacy(xs)
        out = {"line_search": self.line_search(xs), "conj_next": nxt, "conj_far": far, "energy_rise": self.energy_rise(xs)}
        if ref is not None:
            out["iterate_error"] = self.iterate_error(xs, ref)
        return out


PER_ITERATE = ("iterate_error", "line_search", "conj_next", "conj_far")


def spread(judge, res_ld, *others):
    """The restatement's own rounding spread of the iterates given (truncate the runs to the iterates that are judged).
    iterate_error: per iterate, the float64 variants measured against the longdouble one, the largest, as a running maximum
    (rounding differences accumulate along a solve).  line_search, conj_next, conj_far: ONE number per metric and case, the largest
    value over all variants and iterates, repeated per iterate.  These three vanish in exact arithmetic, so every variant's value
    is itself a rounding deviation; each is the projection of accumulated rounding noise on a direction, which a single draw may
    put near zero at a single iterate, so a per-iterate spread of a few draws is no bound for another evaluation
    (tests/test_pcg_oracle_cpu.py shows float64 variants outside the family breaking ten times such a spread, no device involved).
    energy_rise: the largest rise over the variants."""
    n = min([len(res_ld["x"])] + [len(r["x"]) for r in others])
    a = judge.all(res_ld["x"][:n])
    cs = [judge.all(r["x"][:n], ref=res_ld["x"][:n]) for r in others]
    out = {"iterate_error": np.maximum.accumulate(np.max([c["iterate_error"] for c in cs], axis=0))}
    for m in ("line_search", "conj_next", "conj_far"):
        out[m] = np.full(len(a[m]), np.max([a[m]] + [c[m] for c in cs])) if len(a[m]) else a[m]
    out["energy_rise"] = max([a["energy_rise"], 0.0] + [c["energy_rise"] for c in cs])
    return out


def gap_spread(judge, rtol, *results):
    """The residual gap of the restatement's own returned solutions (zero in exact arithmetic): the largest over the variants
    given, floored at one unit round-off in units of rtol."""
    return max(judge.residual_gap(r["x"][r["count"]], r["resid"], rtol) for r in results) + 2.0 ** -53 / rtol


def worst_ratio(values, spread_k):
    """max over the iterates of value / spread (spread floored at one unit round-off of the metric's scale, 2^-53)."""
    if not len(values):
        return 0.0
    s = np.maximum(np.asarray(spread_k[:len(values)], dtype=np.float64), 2.0 ** -53)
    v = np.asarray(values, dtype=np.float64)
    return float(np.max(np.where(np.isfinite(v), v, np.inf) / s))


# ----------------------------------------------------------------------------------------------------------------------
# the inputs of the CPU and GPU tests (chosen on the CPU: tests/test_pcg_oracle_cpu.py checks the band condition on them)
# ----------------------------------------------------------------------------------------------------------------------
# name -> (nz, nr) of start_vector_oracle.lattice_case, or None for the 1960-node fixture.  The sizes are the smallest at which
# each schedule of the update kernels exists (grid_shape): see tests/test_gpu_pcg_loops.py.
MESHES = {"tiny": (9, 13), "fixture": None, "below": (49, 49), "above": (40, 60), "l134": (133, 133), "l513": (512, 512)}


# the boundary vector (index into g_all) each mesh is solved to: chosen so that the band condition holds at rtol 1e-6 and 1e-10
STEP = {"tiny": 1, "fixture": 0, "below": 0, "above": 0, "l134": 0, "l513": 0}


def mesh_case(name):
    """The case dict of start_vector_oracle (coords, tris, tags, tk, trc, dofs, dt, u0, g_all) with three boundary vectors."""
    import start_vector_oracle as so

    if MESHES[name] is None:
        return so.fixture_case(3)
    nz, nr = MESHES[name]
    return so.lattice_case(nz, nr, 3, nbc=min(23, (nz + 1) * (nr + 1) // 6))


def system_of(case, op, A, step=0, u=None, g=None):
    """(b, x0, D^-1) of the step from state u (default: the case's u0) to the boundary values g (default: g_all[step]) on the
    operator A (the device's, or op.Ahat on the CPU): b = start_vector_oracle.rhs_of_step, x0 = u with the boundary values set."""
    import start_vector_oracle as so

    u = np.asarray(case["u0"] if u is None else u, dtype=np.float64)
    g = np.asarray(case["g_all"][step] if g is None else g, dtype=np.float64)
    b, _ = so.rhs_of_step(op, u, g)
    x0 = u.copy()
    x0[op.dofs] = g
    return b, x0, 1.0 / sp.csr_matrix(A).diagonal()


# -- batched columns: built to differ.  SEEDS[(mesh, kind, loop)][j]: the draw of column j's scattered signs (an odd column scales
# its amplitude by 1 + 0.37 draw), raised from 0 only where the restatement would otherwise put a tested residual inside the band
# (Jacobi: tests/test_pcg_oracle_cpu.py checks every column listed in BATCH_CASES; multigrid: the GPU test checks the device's blob)
SEEDS = {("fixture", "percol", "jacobi"): {9: 1, 14: 1}, ("fixture", "affine", "jacobi"): {2: 1}, ("l134", "shared", "jacobi"): {3: 1, 11: 1},
         ("l134", "affine", "jacobi"): {3: 1, 14: 1}, ("l134", "percol", "amg"): {2: 1, 9: 1},
         ("fixture", "percol", "amg"): {14: 1}}
BATCH_CASES = [("fixture", 16, "shared"), ("fixture", 16, "percol"), ("fixture", 16, "affine"),
               ("l134", 16, "shared"), ("l134", 16, "percol"), ("l134", 16, "affine")]     # (nv = 2: the first two columns of these)


def batch_kappas(k0, nv, kind):
    """The conductivity of the re-valued material per column: shared - one operator; percol - k0 (1 + j / 25); affine - k0 (0.88 + j / 25)
    (a stiffer column takes more Jacobi iterations: the factors keep the slowest column of sixteen near the fastest)."""
    if kind == "shared":
        return [k0] * nv
    if kind == "percol":
        return [k0 * (1.0 + 0.04 * j) for j in range(nv)]
    return [k0 + d for d in k0 * (0.04 * np.arange(nv) - 0.12)]


def batch_tag(case):
    """The material the per-column and affine operators re-value: the one with the most cells."""
    return int(np.bincount(np.asarray(case["tags"])).argmax())


def batch_columns(case, nv, kind, mesh, loop="jacobi"):
    """[(u_j, g_j)]: column 0 sits at its solution (a constant field with the same constant on the boundary: no iteration); odd
    columns start close to it (the constant plus the case's u0 scaled by 1e-1 .. 1e-4: the tolerance is relative to b, so a small
    start residual is an easy solve); even columns jump from u0 to ten times another boundary vector with scattered signs (a rough
    right-hand side: hard)."""
    seeds = SEEDS.get((mesh, kind, loop), {})
    cols = []
    for j in range(nv):
        s = seeds.get(j, 0)
        if j == 0:
            cols.append((np.full(len(case["coords"]), 7.0), np.full(len(case["dofs"]), 7.0)))
        elif j % 2:
            amp = 10.0 ** -(1 + (j // 2) % 4) * (1.0 + 0.37 * s)
            cols.append((7.0 + amp * case["u0"], np.full(len(case["dofs"]), 7.0)))
        else:
            sign = np.where(np.random.default_rng(100 * s + j).random(len(case["dofs"])) < 0.5, -1.0, 1.0)
            cols.append((case["u0"], 10.0 * case["g_all"][2] * sign))
    return cols
