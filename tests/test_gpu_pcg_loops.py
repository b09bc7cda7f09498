"""The two PCG loops iterate by iterate (pcg_solve with k_pcg_begin / k_pcg_update / k_pcg_update_amg and the iteration heads
launch_spmv<9>, <2>, <5>; BatchOps::pcg_run with kb_begin / kb_update / kb_reduce) against the float64 / longdouble restatement of
tests/pcg_oracle.py, which tests/test_pcg_oracle_cpu.py judges first.  Every other test sees these loops through their converged
result only, where a wrong beta, a late or mis-scaled convergence test, a column that goes on after it froze or a non-symmetric
cycle cost iterations and nothing else.

The iterates are read without a new entry point: hf_step(..., max_it = k) launches exactly k iterations in every branch of
pcg_solve, returns HF_ERR_NOCONV (HF_OK when iterate k happens to be the converged one of a multigrid solve, whose test runs inside
iteration k) and leaves x_k in the state; a failed step stores nothing in the projection ring, hf_set_state puts the context back.
With hf_set_start_vector(0), x_0 is u with the boundary values set.  The batched loop: hf_batch_run of one step, then
hf_batch_get_state(j).  The loops are bitwise reproducible, so the x_k of k separate truncated solves are the iterates of one
solve - asserted here (the full solve against the last probe, a probe on a fresh context against one after a full solve).

What a truncated probe does NOT return as one might expect (read from the code, confirmed here): the Jacobi loop and the loop of a
one-level hierarchy test iterate k in the head of iteration k + 1, so a probe cut at k = count comes back "not converged" with
iters = count and with the residual of iterate k - 1 in `resid` (hf_step reports the last zz a head summed); the polled multigrid loop
tests iterate k inside iteration k and reports its residual.  Only the residual of a full solve is compared.

Meshes (P = min(ceil(n / 256), 1024) workgroups of the update kernels, a multiple of 8 from 64 on; pcg_oracle.MESHES):
  tiny     10 x 14 = 140         one workgroup, n mod 256 != 0; the hierarchy has one level (copied-back bursts, launch_spmv<4>)
  fixture  1960                  P = 8: one chunk or none per XCD group; multigrid with HEATFLOW_AMG_COARSE = 400 (several levels)
  below    50 x 50 = 2500        the largest one-level hierarchy: build_amg stops at coarse_size = 2500 rows, not at a few dozen
  above    41 x 61 = 2501        the smallest with two levels: the polled loop with held-back cycles
  l134     134 x 134 = 17956     71 chunks on P = 64: some workgroups take two chunks, the last XCD group is short; nv = 16
  l513     513 x 513 = 263169    1029 chunks on P = 1024: the grid-stride second pass; single runs and nv = 2

Bounds.  Counts are equalities, asserted only when every restated tested residual up to the count lies outside [tol / 1.01,
1.01 tol] (a case inside the band fails).  iterate_error, line_search, conj_next, conj_far: at every iterate at most 10 x the
restatement's own spread (the six evaluations of pcg_oracle.VARIANTS, computed per case from the device's own operator and
hierarchy: pcg_oracle.spread - per iterate as a running maximum for iterate_error, one number per case for the other three, whose
per-iterate spread bounds not even another float64 evaluation of the restatement); energy: no rise beyond 10 x the spread's (0:
one unit round-off); residual_gap: 10 x the restatement's.  Mutation floors (tests/test_pcg_oracle_cpu.py): the weakest fault a
metric catches moves it to 3.2e+11 x bound (iterate_error), 2.0e+03 x (line_search), 5.7e+05 x (conj_next), 3.4e+05 x (conj_far),
5.9e+15 x (energy), 2.9e+04 x (gap); the faults of the stopping rule are caught by the count, a frozen column that goes on by the
freeze check.  The batched columns are restated from the device's own right-hand side (read from the projection ring after the full
solve and checked against rhs_of_step to 1e-12 of the row's terms): an easy column starts where b - A x0 cancels to 1e-4 |b| and
less, which enlarges last-place differences between two assemblies of b ten thousand times; the single runs take rhs_of_step's b.
The fused forms of the finest level exist where level 1 reaches HEATFLOW_STREAM_MIN_ROWS rows (default 20000), which the library reads
once per process: the 263169-node lattice has them in this process, the 17956-node lattice runs them in a child process that
starts with HEATFLOW_STREAM_MIN_ROWS = 1000 (the form is asserted from the exported hierarchy in every case), the fixture's level 1
is below any such setting's use and has the explicit form only.
Deviations from the list of cases, for the time a test may take: Jacobi is probed iterate by iterate to K = 12 and then at its
count (multigrid, one level included, at every iterate up to its count); the 263169-node lattice is batched with the shared
operator only (a per-column or affine pair would need a second oracle operator and a second sparse factorisation of 263169 rows,
about 8 s); with nv = 2 the columns are the one at its solution and an easy one, the hard columns exist at nv = 16.

Measured on an MI355X (worst over this file, as multiples of the bound; profiles/pcg_loops_gpu_tests.txt holds every case): every
count equal to the restated one (0 to 142 iterations); iterate_error 0.54 x bound (l134, nv 16, affine, multigrid; as a number at
most 1.5e-09 of |x* - x0| in an easy column, 9.4e-16 in the single runs), line_search 0.46 x, conj_next 0.26 x, conj_far 0.13 x,
energy: no rise, residual_gap 0.015 x; every freeze and bit-for-bit comparison held.  No defect found.
The hand mutation the issue names - a scratch build whose k_pcg_update_amg reads part_rz + (parity ^ 1) * MAXP - fails all five
single-run multigrid tests it was run on, but at their first full solve: on the device that slot is unset at iteration 0 and the
loop diverges ("not converged in 20000 iterations") or breaks down, which any test of a converged result would have seen too.  That
run therefore does not exercise the iterate-level metrics; what shows that they hold the net is the mutation table of
tests/test_pcg_oracle_cpu.py, where the restated faults converge (beta_parity: 152 against 142 iterations) and are caught."""
import numpy as np
import pytest

import pcg_oracle as po
import start_vector_oracle as so
import vcycle_oracle as vo

pytestmark = pytest.mark.gpu

K_JACOBI = 12
FLOORS = {"iterate_error": 3.2e11, "line_search": 2.0e3, "conj_next": 5.7e5, "conj_far": 3.4e5, "energy_rise": 5.9e15, "gap": 2.9e4}


def test_grid_shapes_of_the_chosen_meshes():
    """The arithmetic of the module docstring, so that a change of the launch shapes shows up here."""
    n = {k: 1960 if v is None else (v[0] + 1) * (v[1] + 1) for k, v in po.MESHES.items()}
    assert n == {"tiny": 140, "fixture": 1960, "below": 2500, "above": 2501, "l134": 17956, "l513": 263169}
    assert [po.grid_shape(n[k]) for k in ("tiny", "fixture", "l134", "l513")] == [(1, 1), (8, 8), (71, 64), (1029, 1024)]


# ----------------------------------------------------------------------------------------------------------------------
# cases (module scope: meshes, oracle operators and direct solutions are built once and left unchanged)
# ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def case_of(name):
    if name not in _cases:
        c = po.mesh_case(name)
        c["op"] = so.Operators(c["coords"], c["tris"], c["tags"], c["tk"], c["trc"], c["dt"], c["dofs"])
        c["step"] = po.STEP[name]
        _cases[name] = c
    return _cases[name]


_lus = {}


def judge(key, A, b, dinv, x0):
    """pcg_oracle.Judge with the factorisation of A shared among the tests of one operator (`key`; the values are compared)."""
    hit = _lus.get(key)
    lu = hit[1] if hit is not None and np.array_equal(hit[0], A.data) else None
    J = po.Judge(A, b, dinv, x0, lu=lu)
    _lus[key] = (A.data.copy(), J.lu)
    return J


def context(hip, c, precond, tk=None, reuse=False):
    be = hip.HeatflowHIP(0)
    be.set_mesh(c["coords"], c["tris"], c["tags"])
    tk = c["tk"] if tk is None else tk
    tags = sorted(tk)
    be.set_materials(tags, [tk[t] for t in tags], [c["trc"][t] for t in tags])
    be.set_dirichlet(c["dofs"])
    be.set_precond(precond, reuse=reuse)
    be.set_start_vector(0)
    be.assemble(c["dt"], hip.ASM_ROW_GATHER)
    return be


def amg_env(monkeypatch, fine_level, coarse=None):
    if fine_level is not None:
        monkeypatch.setenv("HEATFLOW_AMG_FUSE0", fine_level)
    if coarse is not None:
        monkeypatch.setenv("HEATFLOW_AMG_COARSE", str(coarse))


def probe(hip, be, u, g, k, rtol, atol=0.0):
    """A solve cut at k iterations from state u: (iters, resid, x_k, converged)."""
    be.set_state(u)
    try:
        it, res = be.step(g, rtol=rtol, atol=atol, max_it=k)
        ok = True
    except hip.NotConverged:
        it, res, ok = be.last_iters, be.last_resid, False
    return it, res, be.get_state(), ok


def judge_iterates(tag, J, xs, rl, rcs, K, brief=False):
    """The per-iterate metrics of the device's x_0..x_K against 10 x the restatement's spread; prints and returns the worst ratios
    to the bound."""
    s = po.spread(J, dict(rl, x=rl["x"][:K + 1]), *[dict(rc, x=rc["x"][:K + 1]) for rc in rcs])
    m = J.all(xs, ref=rl["x"][:K + 1])
    worst = {k: po.worst_ratio(m[k], s[k]) / 10.0 for k in po.PER_ITERATE}
    worst["energy_rise"] = max(m["energy_rise"], 0.0) / (10.0 * max(s["energy_rise"], 2.0 ** -53))
    peak = {k: float(np.max(m[k])) if len(m[k]) else 0.0 for k in po.PER_ITERATE}
    if brief:
        print(f"PCG {tag}: K {K}  " + "  ".join(f"{k} {peak[k]:.1e} = {worst[k]:.2g}" for k in po.PER_ITERATE) + "  (x bound)")
    else:
        print(f"PCG {tag}: K {K}  " + "  ".join(f"{k} {peak[k]:.1e} = {worst[k]:.2g} x bound (floor {FLOORS[k]:.1e} x)" for k in po.PER_ITERATE)
              + f"  energy_rise {m['energy_rise']:.1e} = {worst['energy_rise']:.2g} x bound")
    return worst


def assert_within(tag, worst):
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, "metrics beyond 10 x the restatement's spread (as multiples of the bound)", bad)


# ----------------------------------------------------------------------------------------------------------------------
# single-run loop
# ----------------------------------------------------------------------------------------------------------------------
SINGLE = [("tiny", "jacobi", None, None), ("fixture", "jacobi", None, None), ("l134", "jacobi", None, None), ("l513", "jacobi", None, None),
          ("tiny", "amg", None, None), ("below", "amg", None, None), ("above", "amg", None, None)] + \
         [("fixture", "amg", "0", 400)] + [(name, "amg", f, None) for name in ("l134", "l513") for f in ("0", "1", "2")]


def restate_single(be, c, loop, rtol, atol=0.0, u=None, g=None, chunk_upto=None):
    """(A, b, x0, D^-1, B, hierarchy, longdouble run, the float64 variants' runs (cut at chunk_upto iterations)) for the context's own
    operator."""
    A, dinv = vo.fine_operator(be)
    b, x0, dinv2 = po.system_of(c, c["op"], A, step=c["step"], u=u, g=g)
    assert np.array_equal(dinv, dinv2)
    H = vo.parse_export(be) if loop == "amg" else None
    B = po.multigrid(H, A, dinv) if loop == "amg" else po.jacobi(dinv)
    rl = po.pcg(A, b, x0, B, dinv, rtol, atol)
    rcs = [po.pcg(A, b, x0, B, dinv, rtol, atol, max_it=rl["count"] if chunk_upto is None else chunk_upto, sums=v) for v in po.VARIANTS[1:]]
    return A, b, x0, dinv, B, H, rl, rcs


def run_single(hip, name, loop, fine_level):
    """One single-run case on a fresh context (the environment is the caller's business)."""
    rtol = 1e-10
    c = case_of(name)
    u, g = c["u0"], c["g_all"][c["step"]]
    with context(hip, c, 1 if loop == "amg" else 0) as be:
        levels = be.amg_info()["levels"] if loop == "amg" else 0
        if loop == "amg":
            assert (levels == 1) == (name in ("tiny", "below")), (name, be.amg_info())
            if fine_level is not None:
                L0 = vo.parse_export(be)["levels"][0]
                form = ((L0["Rt"] is not None), (L0["GP"] is not None))
                assert form == {"0": (False, False), "1": (True, True), "2": (True, False)}[fine_level], (name, fine_level, form, be.amg_info())
        polled = loop == "amg" and levels > 1
        K = K_JACOBI if loop == "jacobi" else None           # multigrid, one level included: every iterate up to the count
        A, b, x0, dinv, B, H, rl, rcs = restate_single(be, c, loop, rtol, chunk_upto=K)
        count = rl["count"]
        K = count if K is None else min(K, count)
        tag = f"{name} {loop} fuse0={fine_level} levels={levels}"
        print()
        assert rl["converged"] and po.near_cut(rl) == [], (tag, "a tested residual of the restatement lies in the band", po.near_cut(rl), rl["ratio"])
        J = judge((name, None), A, b, dinv, x0)
        kf = min(3, K)
        fresh = probe(hip, be, u, g, kf, rtol)                           # pred = 0: looks before launching, then one at a time
        be.set_state(u)
        it_full, res_full = be.step(g, rtol=rtol)
        x_full = be.get_state()
        again = probe(hip, be, u, g, kf, rtol)                           # pred = count: a blind burst
        assert fresh[0] == again[0] == kf and np.array_equal(fresh[2], again[2]), (tag, "fresh context against blind burst")
        xs, ks = [x0], list(range(1, K + 1))
        for k in ks:
            it, _, xk, ok = probe(hip, be, u, g, k, rtol)
            assert it == k and ok == (polled and k == count), (tag, k, it, ok)
            xs.append(xk)
        last = xs[-1] if K == count else probe(hip, be, u, g, count, rtol)[2]
        assert it_full == count, (tag, "count", it_full, count)
        assert np.array_equal(x_full, last), (tag, "the full solve is not the last probe bit for bit")
        ends = [rl] + ([r for r in rcs if r["converged"]] or [po.pcg(A, b, x0, B, dinv, rtol, sums="chunk")])
        gap = J.residual_gap(x_full, res_full, rtol) / (10.0 * po.gap_spread(J, rtol, *ends))
        worst = judge_iterates(tag, J, xs, rl, rcs, K)
        worst["gap"] = gap
        print(f"PCG {tag}: count {it_full} = {count}, resid {res_full:.3e} (restated {rl['resid']:.3e}), gap {gap:.2g} x bound (floor {FLOORS['gap']:.1e} x)")
        assert_within(tag, worst)


# the fused forms of the finest level exist where level 1 reaches HEATFLOW_STREAM_MIN_ROWS rows (default 20000), which the library reads
# once per process: the 17956-node lattice (level 1: a few thousand rows) runs them in a child process that has the setting from its start
IN_CHILD = {("l134", "1"), ("l134", "2")}


@pytest.mark.parametrize("name,loop,fine_level,coarse", SINGLE, ids=[f"{a}-{b}-{c}" for a, b, c, _ in SINGLE])
def test_single_run_loop_iterate_by_iterate(hip, monkeypatch, tmp_path, name, loop, fine_level, coarse):
    if (name, fine_level) not in IN_CHILD:
        amg_env(monkeypatch, fine_level, coarse)
        run_single(hip, name, loop, fine_level)
        return
    import os
    import subprocess
    import sys

    from conftest import ROOT

    script = tmp_path / "case.py"
    script.write_text(
        "import sys\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "from heatflow_amd import hip_backend as hip\n"
        "import test_gpu_pcg_loops as t\n"
        f"t.run_single(hip, {name!r}, {loop!r}, {fine_level!r})\n")
    env = dict(os.environ, HEATFLOW_STREAM_MIN_ROWS="1000", HEATFLOW_AMG_FUSE0=fine_level)
    res = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    print(res.stdout, end="")
    assert res.returncode == 0, (name, fine_level, res.returncode, res.stderr[-3000:])
    assert f"PCG {name} {loop} fuse0={fine_level}" in res.stdout


@pytest.mark.parametrize("name,loop,coarse", [("fixture", "jacobi", None), ("above", "amg", None), ("fixture", "amg", 400), ("below", "amg", None)])
def test_stopping_rule_counts(hip, monkeypatch, name, loop, coarse):
    """rtol 1e-6 and 1e-10, and an absolute tolerance that decides (ATOL_FACTOR x rtol x |D^-1 b|: the restated count under it must
    differ from the count under rtol alone); the count equals the restatement's and the reported residual is the true one."""
    c = case_of(name)
    amg_env(monkeypatch, None, coarse)
    u, g = c["u0"], c["g_all"][c["step"]]
    with context(hip, c, 1 if loop == "amg" else 0) as be:
        counts = {}
        for rtol, factor in ((1e-6, 0.0), (1e-10, 0.0), (1e-10, po.ATOL_FACTOR)):
            A, b, x0, dinv, B, H, rl, _ = restate_single(be, c, loop, rtol, chunk_upto=1)
            atol = factor * rtol * np.sqrt(rl["bn2"])
            if factor:
                A, b, x0, dinv, B, H, rl, _ = restate_single(be, c, loop, rtol, atol, chunk_upto=1)
                assert rl["tol"] == atol
            assert rl["converged"] and po.near_cut(rl) == [], (name, loop, rtol, factor, po.near_cut(rl), rl["ratio"])
            be.set_state(u)
            it, res = be.step(g, rtol=rtol, atol=atol)
            J = judge((name, None), A, b, dinv, x0)
            rc = po.pcg(A, b, x0, B, dinv, rtol, atol, sums="chunk")
            gap = J.residual_gap(be.get_state(), res, rtol) / (10.0 * po.gap_spread(J, rtol, rl, rc))
            print(f"PCG stop {name} {loop} rtol {rtol:g} atol factor {factor:g}: count {it} = {rl['count']}, resid {res:.3e}, gap {gap:.2g} x bound")
            assert it == rl["count"] and gap <= 1.0, (name, loop, rtol, factor, it, rl["count"], gap)
            counts[(rtol, factor)] = it
        assert counts[(1e-10, po.ATOL_FACTOR)] < counts[(1e-10, 0.0)] and counts[(1e-6, 0.0)] < counts[(1e-10, 0.0)], counts


@pytest.mark.parametrize("name,loop", [("fixture", "jacobi"), ("above", "amg"), ("below", "amg")])
def test_a_start_at_the_solution_takes_no_iteration_and_leaves_the_state(hip, name, loop):
    """A constant field with the same constant on the boundary solves its step exactly (K 1 = 0): iters == 0 and the state unchanged
    bit for bit - on a fresh context (pred = 0: the loop looks before it launches) and after an ordinary solve (pred > 0: a blind burst is
    launched, whose kernels must all return at once)."""
    c = case_of(name)
    u = np.full(len(c["coords"]), 7.0)
    g = np.full(len(c["dofs"]), 7.0)
    with context(hip, c, 1 if loop == "amg" else 0) as be:
        for stage in ("fresh", "after a solve"):
            be.set_state(u)
            it, res = be.step(g, rtol=1e-10)
            assert it == 0 and np.array_equal(be.get_state(), u) and res <= 1e-10, (name, loop, stage, it, res)
            be.set_state(c["u0"])
            it, _ = be.step(c["g_all"][c["step"]], rtol=1e-10)
            assert it > 3


# ----------------------------------------------------------------------------------------------------------------------
# batched loop
# ----------------------------------------------------------------------------------------------------------------------
def batch_probe(hip, be, cols, k, rtol):
    nv = len(cols)
    for j, (u, _) in enumerate(cols):
        be.batch_set_state(j, u)
    g = np.stack([gj for _, gj in cols], axis=1)[None]
    try:
        be.batch_run(g, rtol=rtol, max_it=k)
        ok = True
    except hip.NotConverged:
        ok = False
    return be.last_run_iters[0].copy(), [be.batch_get_state(j) for j in range(nv)], ok


BATCH = [("fixture", nv, kind, loop) for nv in (2, 16) for kind in ("shared", "percol", "affine") for loop in ("jacobi", "amg")] + \
        [("l134", 16, kind, loop) for kind in ("shared", "percol", "affine") for loop in ("jacobi", "amg")] + \
        [("l513", 2, "shared", loop) for loop in ("jacobi", "amg")]


@pytest.mark.parametrize("name,nv,kind,loop", BATCH, ids=[f"{a}-nv{b}-{c}-{d}" for a, b, c, d in BATCH])
def test_batched_loop_iterate_by_iterate(hip, monkeypatch, name, nv, kind, loop):
    rtol = 1e-10
    c = case_of(name)
    amg_env(monkeypatch, None, 400 if name == "fixture" else None)
    cols = po.batch_columns(c, nv, kind, name, loop)
    tag_m = po.batch_tag(c)
    k0 = c["tk"][tag_m]
    with context(hip, c, 1 if loop == "amg" else 0, reuse=True) as be:
        # -- the columns' operators: the device's own A_j (read back after each re-valuation) and the oracle's for the right-hand side
        kjs = po.batch_kappas(k0, nv, kind)
        code = {"shared": hip.BATCH_SHARED, "percol": hip.BATCH_PER_COLUMN, "affine": hip.BATCH_AFFINE}[kind]
        if kind == "shared":
            fine = [vo.fine_operator(be)] * nv
            be.batch_begin(nv, code)
        elif kind == "percol":
            fine = []
            be.batch_begin(nv, code)
            for j in range(nv):
                be.update_kappa([tag_m], [kjs[j]])
                fine.append(vo.fine_operator(be))
                be.batch_load_column(j)
        else:
            deltas = np.array(kjs) - k0
            fine = []
            for j in range(nv):
                be.update_kappa([tag_m], [kjs[j]])
                fine.append(vo.fine_operator(be))
            be.update_kappa([tag_m], [k0])
            be.batch_begin(nv, code)
            be.batch_set_affine([tag_m], deltas)
        H = vo.parse_export(be) if loop == "amg" else None
        ops = {}
        for kj in kjs:
            if kj not in ops:
                ops[kj] = c["op"] if kj == k0 else so.Operators(c["coords"], c["tris"], c["tags"], {**c["tk"], tag_m: kj}, c["trc"], c["dt"], c["dofs"])
        # -- a probe on the fresh batch (pred = 0), then the full solve: it leaves every column's right-hand side in the projection ring
        fresh = batch_probe(hip, be, cols, 3, rtol)
        it_full, x_full, ok = batch_probe(hip, be, cols, 20000, rtol)
        assert ok
        # -- the restatement, column by column (independent columns; each stops changing at its own count).  Its right-hand side is
        # the device's own b_j, checked against rhs_of_step to 1e-12 of the row's terms (the agreement the parity tests ask of M and
        # A): an easy column starts with |b - A x0| = 1e-4 |b| and less, where last-place differences between two assemblies of b would
        # reach the iterates 1e4 times enlarged - they belong to the assembly, which has its own tests, not to the loop
        R, in_band = [], []
        for j, (u, g) in enumerate(cols):
            A, dinv = fine[j]
            b_ref, x0, _ = po.system_of(c, ops[kjs[j]], A, u=u, g=g)
            _, mag = so.rhs_of_step(ops[kjs[j]], u, g)
            snap = be.get_projection(column=j, arrays=True)
            b = snap["F"][snap["pending"]].copy()
            assert (np.abs(b - b_ref) <= 1e-12 * mag).all(), (name, kind, j, "right-hand side", float((np.abs(b - b_ref) / np.maximum(mag, 1e-300)).max()))
            B = po.multigrid(H, A, dinv, explicit=True) if loop == "amg" else po.jacobi(dinv)
            rl = po.pcg(A, b, x0, B, dinv, rtol)
            K = rl["count"] if loop == "amg" else min(K_JACOBI, rl["count"])
            rcs = [po.pcg(A, b, x0, B, dinv, rtol, max_it=K, sums=v) for v in po.VARIANTS[1:]] if rl["count"] else []
            assert rl["converged"]
            if po.near_cut(rl):
                in_band.append((j, po.near_cut(rl), rl["ratio"][-2:]))
            R.append({"A": A, "b": b, "x0": x0, "dinv": dinv, "rl": rl, "rcs": rcs, "K": K})
        assert not in_band, (name, nv, kind, loop, "tested residuals of the restatement inside the band (column, iterates, last ratios)", in_band)
        counts = np.array([r["rl"]["count"] for r in R])
        assert counts[0] == 0 and len(set(counts.tolist())) >= min(nv, 3), counts
        assert np.array_equal(it_full, counts), (name, nv, kind, loop, "counts", it_full, counts)
        # -- probes 1..K (multigrid: K = the slowest column's count) and at every distinct count
        K = int(counts.max()) if loop == "amg" else K_JACOBI
        ks = sorted(set(range(1, K + 1)) | set(int(v) for v in counts if v > 0))
        again = batch_probe(hip, be, cols, 3, rtol)                         # pred = the slowest column's count: a blind burst
        assert np.array_equal(fresh[0], again[0]) and all(np.array_equal(a, b_) for a, b_ in zip(fresh[1], again[1])), "fresh batch against blind burst"
        P = {}
        for k in ks:
            it, xk, ok = batch_probe(hip, be, cols, k, rtol)
            assert np.array_equal(it, np.minimum(counts, k)), (name, nv, kind, loop, k, it, counts)
            assert ok == (loop == "amg" and k >= counts.max()), (name, nv, kind, loop, k, ok)
            P[k] = xk
        tagb = f"batch {name} nv={nv} {kind} {loop}"
        print()
        worst_all = {}
        for j, r in enumerate(R):
            cj = int(counts[j])
            # freeze: from its count on, column j is the iterate of probe count_j (count 0: the start vector) bit for bit
            frozen = r["x0"] if cj == 0 else P[cj][j]
            for k in ks:
                if k >= cj:
                    assert np.array_equal(P[k][j], frozen), (tagb, "column", j, "changed after it froze: probe", k, "count", cj)
            assert np.array_equal(x_full[j], frozen), (tagb, "column", j, "full solve against the probe at its count")
            if cj == 0:
                continue
            Kj = min(r["K"], K)
            xs = [r["x0"]] + [P[k][j] for k in range(1, Kj + 1)]
            J = judge((name, None if kind == "shared" else (kind, j)), r["A"], r["b"], r["dinv"], r["x0"])
            w = judge_iterates(f"{tagb} column {j} count {cj}", J, xs, r["rl"], r["rcs"], Kj, brief=True)
            for key, v in w.items():
                worst_all[key] = max(worst_all.get(key, 0.0), v)
        print(f"PCG {tagb}: counts {counts.tolist()}  worst over the columns, x bound: " + "  ".join(f"{k} {v:.2g}" for k, v in worst_all.items()))
        assert_within(tagb, worst_all)
        be.batch_end()
