"""The restatement of the PCG loops (tests/pcg_oracle.py) is judged here, on the CPU, before the device is judged against it
(tests/test_gpu_pcg_loops.py).

Cases: Jacobi on the 1960-node fixture and on the lattices of pcg_oracle.MESHES (operators of start_vector_oracle.Operators, the
right-hand side of rhs_of_step, x0 = u0 with the boundary values set), and multigrid on hierarchies built by amg_host.hpp on the
model operator of tests/cpp/vcycle_levels_dump.cpp (64 x 50 rows, the three forms of the finest level).  The restated PCG must
reach the direct solution, its longdouble and chunked-float64 variants must agree (their difference is the spread the GPU bounds
are ten times of) and take the same number of iterations, the inputs of the GPU tests must keep every tested residual outside
the band [tol / 1.01, 1.01 tol], and every named mutation must move a metric.

Spread of the restatement over pcg_oracle.VARIANTS (longdouble with every statement rounded once, against float64 sums in 256-, 64-
and 1024-row chunks, pairwise, and 256-row chunks with longdouble row sums of A v), worst over these cases, first 12 iterates / whole
solve at rtol 1e-10 (printed as SPREAD by the first two tests):
  iterate_error  8.4e-16 / 8.4e-16                  line_search  8.1e-15 / 1.2e-06 (Jacobi), 5.3e-11 / 2.5e-05 (multigrid)
  conj_next      2.7e-15 / 6.1e-08, 3.7e-13 / 7.7e-08      conj_far     2.5e-14 / 2.4e-07, 3.1e-13 / 2.0e-07
  energy_rise    0 (the energy fell at every iterate of every run)       residual_gap  at most 5.3e-07 rtol
line_search and the conjugacies are angles against the TRUE residual b - A x_{k+1} and between search directions, which lose their
orthogonality as rounding accumulates: they grow along a solve.  Each is a projection of rounding noise on a direction, so one draw
may come out near zero at one iterate; pcg_oracle.spread therefore keeps ONE number per metric and case for them (the largest over
variants and iterates) and a per-iterate running maximum for iterate_error only
(test_a_sum_outside_the_family_stays_within_ten_times_the_spread).

Mutation table (printed by test_each_mutation_moves_a_metric; -s shows it).  Each entry is the worst ratio of the mutated run's
metric to the GPU bound (10 x the spread; whole solves at rtol 1e-10, Jacobi on the fixture, multigrid on the 64 x 50 model operator
with the explicit finest level), count = the mutated count against the restated one, gap = residual_gap over its bound.  A metric
catches a mutation when its ratio is at least 100; inf = the mutated run diverged.

  mutation                           iter_err  line_srch  conj_next   conj_far     energy  count     gap        caught by
  jacobi: (none, chunked variant)     1.0e-01    9.9e-02    1.0e-01    1.0e-01    0.0e+00   142/142   1.9e-02   UNSEEN
  jacobi: beta_parity                 2.4e+13    4.3e-05    1.2e+07    6.4e+05    0.0e+00   152/142   2.1e-02   iterate_error, conj_next, conj_far, count
  jacobi: alpha_stale                 1.1e+17    3.4e+05    1.2e+07    6.6e+05    3.3e+16   152/142   0.0e+00   iterate_error, line_search, conj_next, conj_far, energy_rise, count
  jacobi: test_on_r                   0.0e+00    8.8e-11    0.0e+00    0.0e+00    0.0e+00     1/142   1.2e+14   count, gap
  jacobi: tol_on_start                0.0e+00    4.3e-02    1.0e-01    1.0e-01    0.0e+00   143/142   4.9e-04   count
  jacobi: test_late                   0.0e+00    4.3e-02    1.0e-01    1.0e-01    0.0e+00   143/142   4.9e-04   count
  multigrid: (none, chunked variant)  1.0e-01    1.0e-01    1.0e-01    1.0e-01    0.0e+00    23/23    5.1e-02   UNSEEN
  multigrid: beta_parity              3.2e+11    7.7e-07    6.2e+05    5.1e+05    0.0e+00    32/23    6.7e-03   iterate_error, conj_next, conj_far, count
  multigrid: alpha_stale              3.1e+14    2.0e+03    1.3e+06    5.1e+05    5.9e+15    33/23    0.0e+00   iterate_error, line_search, conj_next, conj_far, energy_rise, count
  multigrid: test_on_r                0.0e+00    5.7e-04    1.0e-01    1.0e-01    0.0e+00    24/23    2.9e+04   count, gap
  multigrid: tol_on_start             0.0e+00    4.1e-05    5.1e-03    1.9e-03    0.0e+00    20/23    9.6e-03   count
  multigrid: test_late                0.0e+00    5.7e-04    1.0e-01    1.0e-01    0.0e+00    24/23    1.7e-02   count
  multigrid: no_post_smoothing        9.5e+12    8.6e-08    5.7e+05    3.4e+05    0.0e+00    33/23    4.3e-02   iterate_error, conj_next, conj_far, count
  batched: batch_frozen_updates (column 2)  0.0e+00    7.9e-02    1.0e-01    1.0e-01    0.0e+00   135/135   4.8e-03   freeze
  batched: batch_alpha_of_next (column 1)      inf        inf        inf    6.6e+05        inf   152/142       inf   iterate_error, line_search, conj_next, conj_far, energy_rise, freeze, count, gap

Mutation floors, as multiples of the bound (the smallest ratio among the mutations a metric catches): iterate_error 3.2e+11,
line_search 2.0e+03, conj_next 5.7e+05, conj_far 3.4e+05, energy_rise 5.9e+15, gap 2.9e+04.  Every bound lies at least 100 times
below its floor.  Unseen by every per-iterate metric, by the nature of the fault: test_on_r, tol_on_start and test_late leave the
iterates of a truncated solve untouched - only the count (and for test_on_r the residual gap) sees them; batch_frozen_updates
leaves every iterate up to the count untouched - only the freeze check sees it.  line_search does not see beta_parity or
no_post_smoothing (a wrong direction still gets its exact step length).  No mutation is unseen by every check."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import pcg_oracle as po
import start_vector_oracle as so
from test_vcycle_oracle_cpu import _read, dump_exe  # noqa: F401  (the fixture that compiles the hierarchy dump with g++)

RTOLS = (1e-6, 1e-10)
CPU_MESHES = ("tiny", "fixture", "below", "above", "l134")
# sanity limit on the residual gap of the restatement itself: the recursive residual carries about 1e-16 / rtol of relative noise
# (1e-6 at rtol = 1e-10); the GPU bound is 10 x the gap measured per case (pcg_oracle.gap_spread), not this number
GAP_SANITY = 1e-5
K_GPU = 12          # the iterates of a Jacobi solve the GPU tests probe one by one


_systems = {}


def jacobi_system(name):
    if name not in _systems:
        c = po.mesh_case(name)
        op = so.Operators(c["coords"], c["tris"], c["tags"], c["tk"], c["trc"], c["dt"], c["dofs"])
        _systems[name] = (c, op)
    return _systems[name]


@pytest.fixture(scope="module")
def hierarchies(dump_exe, tmp_path_factory):  # noqa: F811
    """{fuse0: (H, A0, D^-1, b, x0)} on the 64 x 50 model operator."""
    out = {}
    d = tmp_path_factory.mktemp("pcg_levels")
    for fuse0 in (0, 1, 2):
        path = str(d / f"levels{fuse0}.bin")
        run = subprocess.run([dump_exe, "64", "50", str(fuse0), path], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0, run.stderr
        A0, levels = _read(path)
        Ac = levels[-1]["A"].toarray()
        H = {"header": {"nl": len(levels), "f32": 0, "coarse_n": Ac.shape[0], "coarse_ld": Ac.shape[0]}, "levels": levels,
             "coarse_inv": np.linalg.inv(Ac)}
        n = A0.shape[0]
        i = np.arange(n)
        rng = np.random.default_rng(4)
        b = np.sin(0.013 * i) + 0.3 * np.cos(0.21 * (i % 64)) + 0.05 * rng.standard_normal(n)
        out[fuse0] = (H, sp.csr_matrix(A0), 1.0 / A0.diagonal(), b, 40.0 * np.cos(0.37 * (i // 64)) * np.sin(0.11 * i))   # (a start residual far above |b|)
    return out


def both_variants(A, b, x0, B, dinv, rtol, atol=0.0, max_it=20000):
    """The longdouble run and the chunked float64 one (the device's shape); all_variants adds the rest of the family."""
    return (po.pcg(A, b, x0, B, dinv, rtol, atol, max_it), po.pcg(A, b, x0, B, dinv, rtol, atol, max_it, sums="chunk"))


def all_variants(A, b, x0, B, dinv, rtol, max_it=20000):
    return [po.pcg(A, b, x0, B, dinv, rtol, 0.0, max_it, sums=v) for v in po.VARIANTS]


def report(tag, judge, rl, *rcs, K=12):
    s = po.spread(judge, rl, *rcs)
    first = po.spread(judge, *[dict(r, x=r["x"][:K + 1]) for r in (rl,) + rcs])
    print(f"SPREAD {tag}: count {rl['count']}  first {K} iterates / whole solve  " + "  ".join(
        f"{m} {first[m][-1]:.1e}/{s[m][-1]:.1e}" for m in po.PER_ITERATE if len(s[m])) + f"  energy_rise {s['energy_rise']:.1e}")
    return s


@pytest.mark.parametrize("rtol", RTOLS)
@pytest.mark.parametrize("name", CPU_MESHES)
def test_restated_jacobi_pcg_reaches_the_direct_solution_and_its_variants_agree(name, rtol):
    c, op = jacobi_system(name)
    A = op.Ahat
    b, x0, dinv = po.system_of(c, op, A, step=po.STEP[name])
    rl, rc, *more = all_variants(A, b, x0, po.jacobi(dinv), dinv, rtol)
    J = po.Judge(A, b, dinv, x0)
    s = report(f"jacobi {name} rtol {rtol:g}", J, rl, rc, *more)
    assert len({r["count"] for r in more} | {rl["count"]}) == 1
    assert rl["converged"] and rc["converged"] and rl["count"] == rc["count"]
    assert po.near_cut(rl) == [] and po.near_cut(rc) == [], (po.near_cut(rl), rl["ratio"][-3:])
    for r in (rl, rc):
        gap = J.residual_gap(r["x"][-1], r["resid"], rtol)
        print(f"   gap {gap:.2e} rtol, |x - x*| / |x* - x0| = {np.abs(r['x'][-1] - J.xstar).max() / J.scale:.2e}")
        assert gap <= GAP_SANITY and r["resid"] <= rtol
        # |D^-1 r| <= rtol |D^-1 b| bounds the error by the condition of D^-1 A (a few hundred here) times rtol
        assert np.abs(r["x"][-1] - J.xstar).max() <= 1e3 * rtol * max(np.abs(J.xstar).max(), J.scale)
    assert s["iterate_error"][min(11, len(s["iterate_error"]) - 1)] <= 1e-14 and s["energy_rise"] == 0.0


@pytest.mark.parametrize("fuse0", [0, 1, 2])
def test_restated_multigrid_pcg_reaches_the_direct_solution_and_its_variants_agree(hierarchies, fuse0):
    H, A, dinv, b, x0 = hierarchies[fuse0]
    B = po.multigrid(H, A, dinv)
    J = po.Judge(A, b, dinv, x0)
    for rtol in RTOLS:
        rl, rc, *more = all_variants(A, b, x0, B, dinv, rtol)
        s = report(f"multigrid fuse0 {fuse0} rtol {rtol:g}", J, rl, rc, *more)
        assert len({r["count"] for r in more} | {rl["count"]}) == 1
        assert rl["converged"] and rl["count"] == rc["count"] and 4 <= rl["count"] <= 25
        assert po.near_cut(rl) == [] and po.near_cut(rc) == [], rl["ratio"]
        gap = J.residual_gap(rl["x"][-1], rl["resid"], rtol)
        print(f"   gap {gap:.2e} rtol")
        assert gap <= GAP_SANITY and rl["resid"] <= rtol
        assert np.abs(rl["x"][-1] - J.xstar).max() <= 1e3 * rtol * np.abs(J.xstar).max()
        assert s["iterate_error"][-1] <= 1e-13 and s["energy_rise"] == 0.0
    # the explicit finest level (the batched cycle) is the same operator: the same count
    assert po.pcg(A, b, x0, po.multigrid(H, A, dinv, explicit=True), dinv, 1e-10)["count"] == rl["count"]


def test_an_absolute_tolerance_decides_the_count_where_the_gpu_tests_use_one():
    """atol = ATOL_FACTOR x |D^-1 b| x rtol ends the solve earlier than rtol alone, outside the band."""
    for name in ("fixture", "above"):
        c, op = jacobi_system(name)
        A = op.Ahat
        b, x0, dinv = po.system_of(c, op, A, step=po.STEP[name])
        plain = po.pcg(A, b, x0, po.jacobi(dinv), dinv, 1e-10)
        atol = po.ATOL_FACTOR * 1e-10 * np.sqrt(plain["bn2"])
        loose = po.pcg(A, b, x0, po.jacobi(dinv), dinv, 1e-10, atol)
        assert loose["count"] < plain["count"] and po.near_cut(loose) == [], (loose["count"], plain["count"])
        assert loose["tol"] == atol


@pytest.mark.parametrize("mesh,nv,kind", po.BATCH_CASES)
def test_batched_columns_of_the_gpu_tests_keep_their_counts_outside_the_band(mesh, nv, kind):
    """Every column the batched GPU tests build (pcg_oracle.batch_columns, on the oracle's operator for the column's conductivity),
    Jacobi at rtol 1e-10: column 0 takes no iteration, the others converge with no tested residual inside the band, and the counts
    differ between columns."""
    c, op = jacobi_system(mesh)
    tag = po.batch_tag(c)
    kjs = po.batch_kappas(c["tk"][tag], nv, kind)
    cols = po.batch_columns(c, nv, kind, mesh)
    ops, counts = {kjs[0]: op} if kind == "shared" else {}, []
    for j, (u, g) in enumerate(cols):
        if kjs[j] not in ops:
            ops[kjs[j]] = so.Operators(c["coords"], c["tris"], c["tags"], {**c["tk"], tag: kjs[j]}, c["trc"], c["dt"], c["dofs"])
        A = ops[kjs[j]].Ahat
        b, x0, dinv = po.system_of(c, ops[kjs[j]], A, u=u, g=g)
        r = po.pcg(A, b, x0, po.jacobi(dinv), dinv, 1e-10, sums="chunk")
        assert r["converged"] and po.near_cut(r) == [], (mesh, kind, j, po.near_cut(r), r["ratio"][-3:])
        counts.append(r["count"])
    print(f"COUNTS {mesh} {kind}: {counts}")
    assert counts[0] == 0 and min(counts[1:]) > K_GPU and len(set(counts)) >= 3 and len(set(counts[:2])) == 2


def test_a_sum_outside_the_family_stays_within_ten_times_the_spread(hierarchies):
    """The bound of the GPU tests is 10 x the spread over pcg_oracle.VARIANTS.  Two further float64 evaluations that are not in
    the family (chunks of 512 and of 100 rows) play the device here: every metric of theirs stays within the bound at every iterate.
    A spread kept per iterate does not bound them: line_search, conj_next and conj_far are projections of rounding noise on a
    direction, which one draw may put near zero at one iterate - measured here up to 2.1 x ten times the per-iterate spread of
    two variants and 1.01 x that of all five, which is why pcg_oracle.spread keeps one number per case for these three."""
    worst = {}
    for fuse0 in (0, 2):
        H, A, dinv, b, x0 = hierarchies[fuse0]
        J = po.Judge(A, b, dinv, x0)
        vs = all_variants(A, b, x0, po.multigrid(H, A, dinv), dinv, 1e-10)
        s = po.spread(J, *vs)
        for outside in po.OUTSIDE:
            r = po.pcg(A, b, x0, po.multigrid(H, A, dinv), dinv, 1e-10, sums=outside)
            n = min(len(r["x"]), len(vs[0]["x"]))
            m = J.all(r["x"][:n], ref=vs[0]["x"][:n])
            for k in po.PER_ITERATE:
                worst[k] = max(worst.get(k, 0.0), po.worst_ratio(m[k], s[k]) / 10.0)
            assert r["count"] == vs[0]["count"]
    print("OUTSIDE the family, x bound:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


# ----------------------------------------------------------------------------------------------------------------------
# mutations
# ----------------------------------------------------------------------------------------------------------------------
def ratios(judge, base_l, spread_, mutated, rtol, base_c=None):
    """Per metric the worst ratio of the mutated run to the GPU bound (10 x spread at the same iterate), + count and gap."""
    n = min(len(mutated["x"]), len(base_l["x"]))
    m = judge.all(mutated["x"][:n], ref=base_l["x"][:n])
    out = {k: po.worst_ratio(m[k], spread_[k]) / 10.0 for k in po.PER_ITERATE}
    rise = m["energy_rise"] if np.isfinite(m["energy_rise"]) else np.inf
    out["energy_rise"] = max(rise, 0.0) / (10.0 * max(spread_["energy_rise"], 2.0 ** -53))
    out["count"] = (mutated["count"], base_l["count"])
    gap = judge.residual_gap(mutated["x"][min(mutated["count"], len(mutated["x"]) - 1)], mutated["resid"], rtol) / (10.0 * po.gap_spread(judge, rtol, base_l, base_c or base_l))
    out["gap"] = gap if np.isfinite(gap) else np.inf
    return out


def line(name, r, extra=()):
    seen = [k for k in po.PER_ITERATE + ("energy_rise",) if r[k] >= 100.0] + list(extra)
    if r["count"][0] != r["count"][1]:
        seen.append("count")
    if r["gap"] >= 100.0:
        seen.append("gap")
    cells = "  ".join(f"{r[k]:9.1e}" for k in po.PER_ITERATE + ("energy_rise",))
    return f"  {name:34s}{cells}  {r['count'][0]:4d}/{r['count'][1]:<4d} {r['gap']:8.1e}   {', '.join(seen) if seen else 'UNSEEN'}", seen


HEAD = f"  {'mutation':34s}" + "  ".join(f"{k:>9s}" for k in ("iter_err", "line_srch", "conj_next", "conj_far", "energy")) + "  count     gap        caught by"


@pytest.mark.filterwarnings("ignore::RuntimeWarning")      # (a mutated run may diverge to inf / nan: that is a catch)
def test_each_mutation_moves_a_metric(hierarchies):
    rtol = 1e-10
    lines, caught = [HEAD], {}
    # -- single-run loop: Jacobi on the fixture, multigrid on the host-built hierarchy (explicit finest level)
    c, op = jacobi_system("fixture")
    A = op.Ahat
    b, x0, dinv = po.system_of(c, op, A)
    H, Am, dm, bm, xm = hierarchies[0]
    systems = {"jacobi": (A, b, x0, dinv, lambda mut: po.jacobi(dinv)),
               "multigrid": (Am, bm, xm, dm, lambda mut: po.cycle_without_post_smoothing(H, Am, dm) if mut == "no_post_smoothing"
                             else po.multigrid(H, Am, dm))}
    for loop, (A_, b_, x_, d_, Bof) in systems.items():
        J = po.Judge(A_, b_, d_, x_)
        rl, rc, *more = all_variants(A_, b_, x_, Bof(None), d_, rtol)
        s = po.spread(J, rl, rc, *more)
        text, seen = line(f"{loop}: (none, chunked variant)", ratios(J, rl, s, rc, rtol, rc))
        lines.append(text)
        assert seen == [], text
        for mut in po.MUTATIONS[:6]:
            if mut == "no_post_smoothing" and loop == "jacobi":
                continue
            res = po.pcg(A_, b_, x_, Bof(mut), d_, rtol, mutation=mut, max_it=rl["count"] + 10)
            text, seen = line(f"{loop}: {mut}", ratios(J, rl, s, res, rtol, rc))
            lines.append(text)
            caught[(loop, mut)] = seen
    # -- batched loop: three Jacobi columns on the fixture - at its solution, easy (the case's step), hard (a ten times larger jump)
    J0 = po.Judge(A, b, dinv, x0)
    g_hard = 10.0 * c["g_all"][1]
    b2, x2, _ = po.system_of(c, op, A, g=g_hard)
    cols = [(b, J0.xstar), (b, x0), (b2, x2)]
    base = po.pcg_batch([po.Column(A, bb, xx, po.jacobi(dinv), dinv, rtol) for bb, xx in cols])
    assert [r["count"] for r in base][0] == 0 and base[1]["count"] != base[2]["count"]
    for mut in po.MUTATIONS[6:]:
        res = po.pcg_batch([po.Column(A, bb, xx, po.jacobi(dinv), dinv, rtol) for bb, xx in cols], mutation=mut,
                           max_it=max(r["count"] for r in base) + 10)
        # the frozen column is judged where one freezes first; the borrowed alpha in column 1, which has a neighbour
        j = 1 if mut == "batch_alpha_of_next" else min((1, 2), key=lambda q: base[q]["count"])
        Jj = po.Judge(A, cols[j][0], dinv, cols[j][1])
        single = all_variants(A, cols[j][0], cols[j][1], po.jacobi(dinv), dinv, rtol)
        s = po.spread(Jj, *single)
        r = ratios(Jj, single[0], s, dict(res[j], x=res[j]["x"][:len(single[0]["x"])]), rtol, single[1])
        moved = any(not np.array_equal(res[j]["x"][k], res[j]["x"][res[j]["count"]]) for k in range(res[j]["count"], len(res[j]["x"])))
        text, seen = line(f"batched: {mut} (column {j})", r, ("freeze",) if moved else ())
        lines.append(text)
        caught[("batched", mut)] = seen
    print("\n".join(lines))
    for (loop, mut), seen in caught.items():
        assert seen, (loop, mut, "no metric sees this mutation")
    assert "conj_next" in caught[("jacobi", "beta_parity")] and "conj_next" in caught[("multigrid", "beta_parity")]
    assert "line_search" in caught[("jacobi", "alpha_stale")] and "line_search" in caught[("multigrid", "alpha_stale")]
    assert "conj_far" in caught[("multigrid", "no_post_smoothing")]
    for mut in ("test_on_r", "tol_on_start", "test_late"):
        for loop in ("jacobi", "multigrid"):
            assert "count" in caught[(loop, mut)], (loop, mut, caught[(loop, mut)])
    assert "freeze" in caught[("batched", "batch_frozen_updates")]
    assert "line_search" in caught[("batched", "batch_alpha_of_next")]
