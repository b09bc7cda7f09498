"""The read-flux projection on the GPU (hf_flux_setup, hf_flux_solve / hf_flux_project / hf_flux_sample, the flux arguments of
hf_batch_run_flux; k_grad_rows in its three address modes and its block-stride loop, the fallback k_grad_rhs, batch_flux_step)
against the float64 / longdouble restatement of tests/flux_oracle.py, which tests/test_flux_oracle_cpu.py judges first.  The
systems are read through hf_get_flux_system (read-only, host code): M1, D^-1 and the right-hand sides as the device holds them.

Meshes (each the smallest that reaches its branch; 256 rows per block of k_grad_rows):
  fixture    1960 nodes: 8 row blocks, the last partial; the batched tests (nv = 2, 4, 8, 16)
  diamond    case_with_diamond_small: the production stack, a field after heated steps
  l134       134 x 134 = 17956 nodes: 71 row blocks; nv = 16
  flipped40  41 x 41 jittered, every other triangle's vertex order reversed (d < 0)
  fan        flipped40 plus a closed 32-fan as a separate component: one row of 33 entries, so no row-gather lists -
             k_grad_rhs and the scalar solves; 1714 nodes, 7 blocks, the last partial
  l724       725 x 725 = 525625 jittered: 2054 blocks on the grid of 2048, the last of 57 rows; right-hand sides and one loose solve only

Bounds.  M1, D^-1: 1e-13 of the row's largest entry (DESIGN section 5's figure for matrix entries).  Right-hand sides:
|b_dev - b_ld|_i <= 1e-13 S_i, the figure the load kernels are held to; the restatement's own float64 evaluations stay below
1e-15 S (tests/test_flux_oracle_cpu.py).  Solves: pcg_oracle's loop on the device's own M1, D^-1, b and warm start; counts are
equalities where no restated tested residual lies within [tol / 1.01, 1.01 tol]; the result lies within 10 x the spread of the six
evaluations of the final iterate, per case.  Closed form: |g - (c_z, c_r)|_2 <= 2 rtol |D^-1 b|_2 / lambda_min(D^-1 M1) at rtol 1e-8
(|e|_2 <= |(D^-1 M1)^-1| |D^-1 r|_2; the factor 2 covers the gap between the recurrence residual and the true one).

The batched path forms one gradient component of every column per solve and keeps only that component's right-hand sides, so the
z right-hand sides of a flux_components = 3 step are taken from a single-run context at the column's state - bit for bit the
same, which test_batched_right_hand_sides_equal_the_single_run_ones asserts for both components first.

The stopping rule with b = 0 exactly (a state reset to uniform) measures against the start residual, so the loop brings the warm
start down by rtol and stops: at rtol = 1e-6 the first run of this file found 3e-6 of the previous gradient in the result (bound:
1e-8).  The library now returns the solution of M1 g = 0 itself (zero_flat_column); the loop's count stays the restated one.

Measured on an MI355X (worst over this file; profiles/flux_gpu_tests.txt holds the run's output): M1 4.2e-16 of the row's largest
entry and symmetric, D^-1 bit for bit 1 / diag; right-hand sides 3.5e-16 S (0.0035 x bound; 8.1e-17 S on the 525625-row lattice,
8.8e-17 S from k_grad_rhs); the same bits from two calls, two contexts, the plain and the two-column layout and every column of
nv = 2, 4, 8, 16; every count equal to the restated one (0 to 55 iterations, none in the band), iterate_error 0.17 x bound;
closed form 0.21 x bound.  Not covered: the projection with the staged SpMV switched off (HEATFLOW_BATCH_LDS = 0 is read once per
process)."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import flux_oracle as fo
import pcg_oracle as po
import start_vector_oracle as so

pytestmark = pytest.mark.gpu

ROW_TOL = fo.ROW_TOL
MAT_TOL = 1e-13
RTOLS = (1e-6, 1e-10)


# ----------------------------------------------------------------------------------------------------------------------
# cases (module scope: meshes, restatements and factorisations are built once and left unchanged)
# ----------------------------------------------------------------------------------------------------------------------
_cases = {}


def case_of(name, request=None):
    """dict(coords, tris, tags, tk, trc, dofs, dt, u0, g_all, O, name); u0 and g_all are offsets from 300 K."""
    if name not in _cases:
        if name == "fixture":
            c = so.fixture_case(3)
        elif name == "l134":
            c = po.mesh_case("l134")
        elif name == "flipped40":
            c = so.lattice_case(40, 40, 3, mesh=lambda nz, nr: fo.jittered_lattice(nz, nr, flipped=True))
        elif name == "fan":
            c = so.lattice_case(40, 40, 3, mesh=lambda nz, nr: fo.with_fan(*fo.jittered_lattice(nz, nr, flipped=True)))
        elif name == "l724":
            coords, tris = fo.jittered_lattice(724, 724)
            c = {"coords": coords, "tris": tris, "tags": np.ones(len(tris), dtype=np.int32)}
        else:
            cfg, stack, mesh = request.getfixturevalue("case_with_diamond_small")
            c = {"coords": mesh.coords, "tris": mesh.tris, "tags": mesh.tags, "problem": (cfg, stack, mesh)}
        c["O"] = fo.FluxOracle(c["coords"], c["tris"])
        c["name"] = name
        _cases[name] = c
    return _cases[name]


def lu_of(c, M):
    """The factorisation of the device's M1 of a case (kept with the values it was made from)."""
    hit = c.get("lu")
    if hit is None or not np.array_equal(hit[0], M.data):
        c["lu"] = (M.data.copy(), spla.splu(sp.csc_matrix(M)))
    return c["lu"][1]


def flux_context(hip, c):
    """Mesh and hf_flux_setup only: what the single-run projection needs."""
    be = hip.HeatflowHIP(0)
    be.set_mesh(c["coords"], c["tris"], c["tags"])
    be.flux_setup()
    return be


def step_context(hip, c, flux=True):
    """A context that can take time steps (Jacobi-PCG, start vector 0)."""
    be = hip.HeatflowHIP(0)
    be.set_mesh(c["coords"], c["tris"], c["tags"])
    tags = sorted(c["tk"])
    be.set_materials(tags, [c["tk"][t] for t in tags], [c["trc"][t] for t in tags])
    be.set_dirichlet(c["dofs"])
    be.set_precond(0)
    be.set_start_vector(0)
    be.assemble(c["dt"], hip.ASM_ROW_GATHER)
    if flux:
        be.flux_setup()
    return be


def heated_state(hip, c, request=None):
    """A field after a few heated steps, computed once per case on the device."""
    if "heated" not in c:
        if "problem" in c:
            from helpers import make_problem

            prob = make_problem(*c["problem"])
            try:
                prob.run(5, time_varying=[prob.bcs[3]])
                c["heated"] = prob.state()
            finally:
                prob.close()
        else:
            with step_context(hip, c, flux=False) as be:
                be.set_state(300.0 + c["u0"])
                for s in range(3):
                    be.step(300.0 + c["g_all"][s], rtol=1e-10, atol=0.0, max_it=20000)
                c["heated"] = be.get_state()
    return c["heated"]


def plateau_field(coords):
    """The rough field with the half z <= mid-height held at one temperature: rows that see only constant triangles."""
    u = fo.rough_field(coords)
    z = coords[:, 0]
    u[z <= 0.5 * (z.min() + z.max())] = 317.25
    return u


def system(be):
    """(M1 as csr, D^-1) of a context."""
    rowptr, colidx, _, _ = be.get_csr(values=False)
    s = be.flux_system(matrix=True, want_z=False, want_r=False)
    return sp.csr_matrix((s["M1"], colidx, rowptr), shape=(be.n, be.n)), s["dinv1"]


def check_rhs(be, O, u, label, components=3):
    """hf_flux_solve (loose) of the state u; the right-hand sides it formed against the longdouble restatement, row by row."""
    be.set_state(u)
    be.flux_solve(1e-2, 5000, want_z=bool(components & 1), want_r=bool(components & 2))
    s = be.flux_system(want_z=bool(components & 1), want_r=bool(components & 2))
    bz, br, Sz, Sr = O.rhs(u)
    worst = 0.0
    for got, ref, S in ((s["bz"], bz, Sz), (s["br"], br, Sr)):
        if got is not None:
            worst = max(worst, fo.row_ratio(got, ref, S))
    print(f"FLUX rhs {label}: max |b - b_ld| / S = {worst:.2e} = {worst / ROW_TOL:.2g} x bound")
    assert worst <= ROW_TOL, label
    return s


def final_spread(J, rl, rcs):
    """pcg_oracle.spread's iterate_error at the last iterate: the float64 evaluations against the longdouble one, the largest over
    the iterates up to the count (rounding differences accumulate along a solve), floored at one unit round-off."""
    n = min([len(rl["x"])] + [len(r["x"]) for r in rcs])
    if n == 0 or not rcs:
        return 2.0 ** -53
    return max(2.0 ** -53, max(float(J.iterate_error(r["x"][:n], rl["x"][:n]).max()) for r in rcs))


def judge_solve(tag, c, M, dinv, b, x0, rtol, got, got_count, rl=None):
    """One solve of the device against the restatement: count (where no tested residual lies in the band) and final iterate."""
    J = po.Judge(M, b, dinv, x0, lu=lu_of(c, M))
    if rl is None:
        rl = fo.solve(M, dinv, b, x0, rtol)
    rcs = [fo.solve(M, dinv, b, x0, rtol, sums=v, max_it=max(rl["count"], 1)) for v in po.VARIANTS[1:]]
    assert rl["converged"], tag
    band = po.near_cut(rl)
    err = float(J.iterate_error([got], [fo.final(rl)])[0])
    bound = 10.0 * final_spread(J, rl, rcs)
    print(f"FLUX solve {tag}: count {got_count} (restated {rl['count']}{', in the band: not asserted' if band else ''})  "
          f"iterate_error {err:.1e} = {err / bound:.2g} x bound")
    if not band:
        assert got_count == rl["count"], (tag, got_count, rl["count"])
    assert err <= bound, (tag, err, bound)
    return err / bound


# ----------------------------------------------------------------------------------------------------------------------
# a. the matrix
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture", "diamond", "l134", "flipped40", "fan"])
def test_mass_matrix_and_its_inverse_diagonal(hip, request, name):
    c = case_of(name, request)
    O = c["O"]
    with flux_context(hip, c) as be:
        rowptr, colidx, _, _ = be.get_csr(values=False)
        assert np.array_equal(rowptr, O.rowptr) and np.array_equal(colidx, O.colidx)
        M, dinv = system(be)
    Mref, dref = O.mass()
    rowmax = np.repeat(np.maximum.reduceat(np.abs(Mref.data), Mref.indptr[:-1]), np.diff(Mref.indptr))
    worst = float((np.abs(M.data - Mref.data) / rowmax).max())
    print(f"FLUX M1 {name}: max |M1 - M1_ld| / row max = {worst:.2e} = {worst / MAT_TOL:.2g} x bound")
    assert worst <= MAT_TOL
    assert abs(M - M.T).max() == 0.0
    assert np.array_equal(dinv, 1.0 / M.diagonal())
    assert np.abs(dinv - dref).max() <= MAT_TOL * np.abs(dref).max()


# ----------------------------------------------------------------------------------------------------------------------
# b. right-hand sides row by row
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture", "diamond", "l134", "flipped40", "fan"])
def test_right_hand_sides_row_by_row(hip, request, name):
    c = case_of(name, request)
    O = c["O"]
    states = {"heated": heated_state(hip, c, request), "linear": fo.linear_field(c["coords"]), "rough": fo.rough_field(c["coords"]),
              "plateau": plateau_field(c["coords"])}
    with flux_context(hip, c) as be:
        assert (np.diff(O.rowptr).max() > 32) == (name == "fan")          # the fan's centre row is what takes k_grad_rhs
        for label, u in states.items():
            s = check_rhs(be, O, u, f"{name} {label}")
            if label == "plateau":
                flat = np.ones(O.n, dtype=bool)
                flat[O.tris[(u[O.tris] != 317.25).any(axis=1)].ravel()] = False
                _, _, Sz, Sr = O.rhs(u)
                assert flat.sum() > O.n // 4
                assert np.all(np.abs(s["bz"][flat]) <= ROW_TOL * Sz[flat]) and np.all(np.abs(s["br"][flat]) <= ROW_TOL * Sr[flat])


def test_block_stride_loop_and_partial_last_block(hip):
    """525625 rows = 2053 x 256 + 57: 2054 row blocks on k_grad_rows' grid of 2048 workgroups, six of them in the second pass of
    the block-stride loop, the last with 57 rows.  Right-hand sides in both layouts and one loose solve, nothing more."""
    c = case_of("l724")
    O = c["O"]
    assert O.n == 525625 and (O.n + 255) // 256 == 2054 and O.n % 256 == 57
    u = fo.rough_field(c["coords"])
    with flux_context(hip, c) as be:
        pair = check_rhs(be, O, u, "l724 rough, two-column layout", 3)
        assert max(be.last_flux_iters) < 50
        plain = {}
        for kw in (dict(want_z=True, want_r=False), dict(want_z=False, want_r=True)):
            be.flux_solve(1e30, 5000, **kw)                    # the plain arrays: formed; at this rtol the solve ends at its start
            assert max(be.last_flux_iters) == 0
            plain.update({k: v for k, v in be.flux_system(**kw).items() if v is not None})
        assert np.array_equal(plain["bz"], pair["bz"]) and np.array_equal(plain["br"], pair["br"])


# ----------------------------------------------------------------------------------------------------------------------
# c. equalities that cost nothing
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture", "flipped40"])
def test_right_hand_sides_are_the_same_bits_in_every_layout_call_and_context(hip, name):
    c = case_of(name)
    u = heated_state(hip, c)
    got = []
    for _ in range(2):
        with flux_context(hip, c) as be:
            be.set_state(u)
            for _ in range(2):
                be.flux_solve(1e-6, 5000)
                got.append(be.flux_system())
            be.flux_solve(1e-6, 5000, want_r=False)
            bz = be.flux_system(want_r=False)["bz"]
            be.flux_solve(1e-6, 5000, want_z=False)
            br = be.flux_system(want_z=False)["br"]
            got.append({"bz": bz, "br": br})
    for s in got[1:]:
        assert np.array_equal(s["bz"], got[0]["bz"]) and np.array_equal(s["br"], got[0]["br"])
    assert np.abs(got[0]["bz"]).max() > 0 and np.abs(got[0]["br"]).max() > 0


def column_inputs(c, nv):
    """Columns built to differ: (states, boundary values (3, n_bc, nv)) as absolute temperatures."""
    sign = np.where(np.arange(nv) % 2 == 0, 1.0, -1.0)
    u = [300.0 + sign[j] * (1.0 + 0.25 * j) * c["u0"] for j in range(nv)]
    g = 300.0 + c["g_all"][:, :, None] * (sign * (1.0 + 0.1 * np.arange(nv)))[None, None, :]
    return u, g


def open_batch(hip, be, c, nv):
    be.batch_begin(nv, per_column_operator=hip.BATCH_SHARED)
    u, g = column_inputs(c, nv)
    for j in range(nv):
        be.batch_set_state(j, u[j])
    return g


def single_rhs(single, u):
    """(b_z, b_r) a single-run context forms at the state u."""
    single.set_state(u)
    single.flux_solve(1e-2, 5000)
    s = single.flux_system()
    return s["bz"], s["br"]


@pytest.mark.parametrize("name,nv", [("fixture", 2), ("fixture", 4), ("fixture", 8), ("fixture", 16), ("l134", 16)])
def test_batched_right_hand_sides_equal_the_single_run_ones(hip, name, nv):
    """Column j of the nv-interleaved state (stride = ustride = nv, uoff = j, one launch per column) against the plain arrays."""
    c = case_of(name)
    O = c["O"]
    nodes = np.arange(0, O.n, 97, dtype=np.int32)
    worst = 0.0
    with step_context(hip, c) as be, flux_context(hip, c) as single:
        g = open_batch(hip, be, c, nv)
        for call, comps in enumerate((1, 2, 3)):
            be.batch_run(g[call:call + 1], 1e-10, 0.0, 20000, None, flux_nodes=nodes, flux_components=comps, flux_rtol=1e-6)
            states = [be.batch_get_state(j) for j in range(nv)]
            assert all(np.abs(states[j] - states[0]).max() > 1e-3 for j in range(1, nv))            # the columns differ
            held = "bz" if comps == 1 else "br"
            for j in range(nv):
                bz, br = single_rhs(single, states[j])
                got = be.flux_system(column=j, want_z=comps == 1, want_r=comps != 1)[held]
                assert np.array_equal(got, bz if comps == 1 else br), (name, nv, comps, j)
                if j in (0, nv - 1):
                    rz, rr, Sz, Sr = O.rhs(states[j])
                    worst = max(worst, fo.row_ratio(got, rz if comps == 1 else rr, Sz if comps == 1 else Sr))
        be.batch_end()
    print(f"FLUX batched rhs {name} nv={nv}: bit for bit the single-run ones; max |b - b_ld| / S = {worst:.2e} = {worst / ROW_TOL:.2g} x bound")
    assert worst <= ROW_TOL


# ----------------------------------------------------------------------------------------------------------------------
# d. the solves
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rtol", RTOLS)
@pytest.mark.parametrize("name,components", [("fixture", 3), ("fixture", 1), ("fixture", 2), ("l134", 3), ("l134", 2), ("fan", 3)])
def test_single_run_solves_against_the_restated_loop(hip, name, components, rtol):
    """The two-column solve (components = 3 with row-gather lists), the scalar solve of one component, the two scalar solves of the
    fallback: a cold solve, a warm-started one, then a state gone uniform (b = 0 exactly on the straight lattice - the bn2 = 0
    stopping rule - and rounding noise on the others, a solve like any other)."""
    c = case_of(name)
    kw = dict(want_z=bool(components & 1), want_r=bool(components & 2))
    states = [heated_state(hip, c), fo.rough_field(c["coords"]), np.full(len(c["coords"]), 300.0)]
    worst = 0.0
    with flux_context(hip, c) as be:
        M, dinv = system(be)
        prev = {"bz": np.zeros(be.n), "br": np.zeros(be.n)}
        for k, u in enumerate(states):
            be.set_state(u)
            g = dict(zip(("bz", "br"), be.flux_project(rtol, 5000, **kw)))
            its = be.last_flux_iters.copy()
            b = be.flux_system(**kw)
            for q, key in enumerate(("bz", "br")):
                if b[key] is None:
                    continue
                tag = f"{name} components={components} rtol={rtol:.0e} solve {k} {key[1]}"
                if k == 2:
                    assert np.abs(g[key]).max() <= 1e-8 * np.abs(prev[key]).max(), tag
                    if not b[key].any():
                        # b = 0 exactly: the loop runs under the bn2 = 0 rule (tol = rtol x the start residual) and brings the warm
                        # start down by rtol only; the library then returns the solution of M1 g = 0 itself
                        rl = fo.solve(M, dinv, b[key], prev[key], rtol)
                        print(f"FLUX solve {tag}: b = 0 exactly, count {its[q]} (restated {rl['count']}), result exactly zero: {not g[key].any()}")
                        assert po.near_cut(rl) or its[q] == rl["count"], (tag, its[q], rl["count"])
                        assert rl["count"] > 0 and not g[key].any(), tag
                        prev[key] = g[key]
                        continue
                worst = max(worst, judge_solve(tag, c, M, dinv, b[key], prev[key], rtol, g[key], int(its[q])))
                prev[key] = g[key]
    print(f"FLUX solves {name} components={components} rtol={rtol:.0e}: worst iterate_error {worst:.2g} x bound")


@pytest.mark.parametrize("rtol", RTOLS)
@pytest.mark.parametrize("components", [1, 2, 3])
@pytest.mark.parametrize("nv", [2, 16])
def test_batched_solves_against_the_restated_loop(hip, nv, components, rtol):
    """Three consecutive one-step hf_batch_run_flux calls with every node sampled: the warm starts of the second and third call are
    the first's and the second's results, each component's own (flux_components = 3: the exchange of F.u and F.uprev)."""
    c = case_of("fixture")
    n = c["O"].n
    nodes = np.arange(n, dtype=np.int32)
    comps = [q for q in (0, 1) if (components >> q) & 1]
    worst = 0.0
    with step_context(hip, c) as be, flux_context(hip, c) as single:
        M, dinv = system(be)
        B = po.jacobi(dinv)
        g = open_batch(hip, be, c, nv)
        prev = np.zeros((len(comps), nv, n))
        for call in range(3):
            _, _, flux = be.batch_run(g[call:call + 1], 1e-10, 0.0, 20000, None, flux_nodes=nodes, flux_components=components, flux_rtol=rtol)
            its = be.last_flux_iters[0].copy()
            rhs = [single_rhs(single, be.batch_get_state(j)) for j in range(nv)]
            for k, q in enumerate(comps):
                cols = [po.Column(M, rhs[j][q], prev[k, j], B, dinv, rtol, 0.0, "ld") for j in range(nv)]
                res = po.pcg_batch(cols, max_it=5000)
                band = [j for j in range(nv) if po.near_cut(res[j])]
                counts = [r["count"] for r in res]
                tag = f"fixture nv={nv} components={components} rtol={rtol:.0e} call {call} {'zr'[q]}"
                print(f"FLUX batched {tag}: flux_iters {its[k]} (restated max {max(counts)}{', columns in the band: ' + str(band) if band else ''})")
                if not band:
                    assert its[k] == max(counts), (tag, its[k], counts)
                for j in range(nv):
                    rl = dict(res[j], x=res[j]["x"][:res[j]["count"] + 1])
                    worst = max(worst, judge_solve(f"{tag} column {j}", c, M, dinv, rhs[j][q], prev[k, j], rtol, flux[0, k, j], counts[j], rl=rl))
            prev = flux[0].copy()
        be.batch_end()
    print(f"FLUX batched solves nv={nv} components={components} rtol={rtol:.0e}: worst iterate_error {worst:.2g} x bound")


# ----------------------------------------------------------------------------------------------------------------------
# e. the closed form
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixture", "flipped40", "l134", "fan"])
def test_linear_field_projects_onto_its_constant_gradient(hip, name):
    c = case_of(name)
    rtol = 1e-8
    lo, _ = c["O"].spectrum()
    with flux_context(hip, c) as be:
        be.set_state(fo.linear_field(c["coords"]))
        gz, gr = be.flux_project(rtol, 5000)
        s = be.flux_system(matrix=True)
    for key, got, coef in (("bz", gz, fo.LIN[1]), ("br", gr, fo.LIN[2])):
        err = float(np.linalg.norm(got - coef))
        bound = 2.0 * rtol * float(np.linalg.norm(s["dinv1"] * s[key])) / lo
        print(f"FLUX closed form {name} d/d{key[1]}: |g - c|_2 = {err:.2e} = {err / bound:.2g} x bound (lambda_min {lo:.4f})")
        assert err <= bound, (name, key)


# ----------------------------------------------------------------------------------------------------------------------
# f. the batched output layout
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [2, 4, 8, 16])
def test_batched_output_layout_and_iteration_counts(hip, nv):
    """flux[step, component, column, node] of a two-step call against every column's own single-run projection, and
    flux_iters[step, component] against the largest restated count of the columns."""
    c = case_of("fixture")
    n = c["O"].n
    nodes = np.arange(n - 1, -1, -1, dtype=np.int32)                     # every node, in an order of the caller's
    rtol = 1e-12
    with step_context(hip, c) as be, step_context(hip, c, flux=False) as twin, flux_context(hip, c) as single:
        M, dinv = system(be)
        B = po.jacobi(dinv)
        g = open_batch(hip, be, c, nv)
        _, _, flux = be.batch_run(g[:2], 1e-10, 0.0, 20000, None, flux_nodes=nodes, flux_components=3, flux_rtol=rtol)
        its = be.last_flux_iters.copy()
        be.batch_end()
        assert flux.shape == (2, 2, nv, n) and its.shape == (2, 2)
        open_batch(hip, twin, c, nv)                                       # the same steps one at a time: the states in between
        prev = np.zeros((2, nv, n))
        for s in range(2):
            twin.batch_run(g[s:s + 1], 1e-10, 0.0, 20000, None)
            states = [twin.batch_get_state(j) for j in range(nv)]
            counts = [[], []]
            for j in range(nv):
                single.set_state(states[j])
                own = single.flux_project(rtol, 5000)
                b = single.flux_system()
                for q, key in enumerate(("bz", "br")):
                    scale = np.abs(own[q]).max()
                    assert np.abs(flux[s, q, j][::-1] - own[q]).max() <= 1e-8 * scale, (nv, s, q, j)
                    res = fo.solve(M, dinv, b[key], prev[q, j][::-1], rtol)
                    counts[q].append(None if po.near_cut(res) else res["count"])
            for q in range(2):
                print(f"FLUX layout nv={nv} step {s} {'zr'[q]}: flux_iters {its[s, q]}, restated counts {counts[q]}")
                if None not in counts[q]:
                    assert its[s, q] == max(counts[q]), (nv, s, q)
            prev = flux[s].copy()
        twin.batch_end()


# ----------------------------------------------------------------------------------------------------------------------
# g. state rules
# ----------------------------------------------------------------------------------------------------------------------
def _state_error(hip, call):
    with pytest.raises(hip.HipError) as e:
        call()
    assert e.value.code == hip.HF_ERR_STATE, e.value
    return str(e.value)


def test_the_window_refuses_what_it_does_not_hold(hip):
    c = case_of("fixture")
    with step_context(hip, c, flux=False) as be:
        _state_error(hip, lambda: be.flux_system(matrix=True, want_z=False, want_r=False))        # before hf_flux_setup
        be.flux_setup()
        assert be.flux_system(matrix=True, want_z=False, want_r=False)["M1"].shape == (be.nnz,)
        _state_error(hip, lambda: be.flux_system(want_r=False))                                      # nothing formed yet
        be.set_state(300.0 + c["u0"])
        be.flux_solve(1e-6, 5000, want_r=False)
        assert be.flux_system(want_r=False)["bz"].any()
        _state_error(hip, lambda: be.flux_system(want_z=False))                                      # r was not formed by that call
        be.flux_solve(1e-6, 5000, want_z=False)
        _state_error(hip, lambda: be.flux_system(want_r=False))
        with pytest.raises(hip.NotConverged):
            be.flux_solve(1e-12, 1)
        assert be.flux_system()["br"].any()                                                          # formed, though not solved
        _state_error(hip, lambda: be.flux_sample(np.arange(3, dtype=np.int32)))
        _state_error(hip, lambda: be.flux_system(column=0, want_r=False))                            # no batch is open
        g = open_batch(hip, be, c, 2)
        _state_error(hip, lambda: be.flux_system(column=0, want_r=False))                            # no batched projection yet
        nodes = np.arange(5, dtype=np.int32)
        be.batch_run(g[:1], 1e-10, 0.0, 20000, None, flux_nodes=nodes, flux_components=3, flux_rtol=1e-6)
        assert be.flux_system(column=1, want_z=False)["br"].any()
        _state_error(hip, lambda: be.flux_system(column=1, want_r=False))                            # the batch holds r
        _state_error(hip, lambda: be.flux_system(column=1))                                          # both
        with pytest.raises(ValueError):
            be.flux_system(column=2, want_z=False)
        be.batch_run(g[1:2], 1e-10, 0.0, 20000, None, flux_nodes=nodes, flux_components=1, flux_rtol=1e-6)
        assert be.flux_system(column=0, want_r=False)["bz"].any()
        _state_error(hip, lambda: be.flux_system(column=0, want_z=False))
        be.batch_end()
        _state_error(hip, lambda: be.flux_system(column=0, want_r=False))
        # a new mesh: everything of the projection is refused until hf_flux_setup is called again
        be.set_mesh(c["coords"], c["tris"], c["tags"])
        _state_error(hip, lambda: be.flux_solve(1e-6, 5000))
        _state_error(hip, lambda: be.flux_sample(nodes))
        _state_error(hip, lambda: be.flux_system())
        be.flux_setup()
        _state_error(hip, lambda: be.flux_sample(nodes))
        be.set_state(300.0 + c["u0"])
        be.flux_solve(1e-6, 5000)
        assert np.isfinite(be.flux_sample(nodes)[0]).all()


def test_batched_projection_is_refused_without_row_gather_lists_and_the_context_goes_on(hip):
    c = case_of("fan")
    with step_context(hip, c) as be:
        g = open_batch(hip, be, c, 2)
        nodes = np.arange(5, dtype=np.int32)
        with pytest.raises(ValueError, match="row-gather lists are not available"):
            be.batch_run(g[:1], 1e-10, 0.0, 20000, None, flux_nodes=nodes, flux_components=3, flux_rtol=1e-6)
        be.batch_run(g[:1], 1e-10, 0.0, 20000, nodes)
        u = be.batch_get_state(1)
        be.batch_end()
        check_rhs(be, c["O"], u, "fan, after the refused call")


def test_failed_r_solve_leaves_both_warm_starts_in_their_places(hip):
    """flux_components = 3 with flux_max_it = 1: the z solve ends at its start (fields that depend on r alone on the straight
    lattice make b_z exactly zero, its warm start is zero), the r solve fails after one iteration and batch_flux_step exchanges
    F.u and F.uprev back.  The next, unrestricted call finds z's warm start (zero: count 0 under the bn2 = 0 rule) and r's (the
    failed solve's first iterate) where they belong; left exchanged, the z solve would start from that iterate with b = 0 and count.
    The time steps run with rtol = 1e30: they end at their start, so the state is what the test set."""
    c = case_of("l134")
    O = c["O"]
    n, nv = O.n, 2
    r = c["coords"][:, 1] / 2.0e-6
    fields = [[300.0 + 40.0 * np.sin(3.0 * r + j) for j in range(nv)], [300.0 + 25.0 * np.cos(5.0 * r - j) + 9.0 * r for j in range(nv)]]
    nodes = np.arange(n, dtype=np.int32)
    rtol = 1e-10

    def run(be, which, **kw):
        for j in range(nv):
            be.batch_set_state(j, fields[which][j])
        g = np.stack([fields[which][j][c["dofs"]] for j in range(nv)], axis=1)[None]
        out = be.batch_run(g, 1e30, 0.0, 20000, None, flux_nodes=nodes, flux_components=3, flux_rtol=rtol, **kw)
        return out[2]

    with step_context(hip, c) as be, flux_context(hip, c) as single:
        M, dinv = system(be)
        be.batch_begin(nv, per_column_operator=hip.BATCH_SHARED)
        first = run(be, 0)
        for j in range(nv):
            assert np.array_equal(be.batch_get_state(j), fields[0][j])
        assert be.last_flux_iters[0, 0] == 0 and not first[0, 0].any() and be.last_flux_iters[0, 1] > 3
        with pytest.raises(hip.NotConverged):
            run(be, 1, flux_max_it=1)
        assert be.last_flux_iters[0, 0] == 0
        second = run(be, 0)
        its = be.last_flux_iters[0].copy()
        assert its[0] == 0 and not second[0, 0].any()
        counts, band = [], False
        for j in range(nv):
            bz1, br1 = single_rhs(single, fields[1][j])
            bz0, br0 = single_rhs(single, fields[0][j])
            assert not bz0.any() and not bz1.any()
            x1 = fo.solve(M, dinv, br1, first[0, 1, j], rtol, max_it=1)["x"][-1]          # where the failed solve stopped
            res = fo.solve(M, dinv, br0, x1, rtol)
            other = fo.solve(M, dinv, br0, np.zeros(n), rtol)
            band = band or bool(po.near_cut(res))
            counts.append((res["count"], other["count"]))
        print(f"FLUX failed r solve: flux_iters after it {its.tolist()}, restated r counts (from the failed solve's iterate, from zero) {counts}")
        if not band:
            assert its[1] == max(k for k, _ in counts)
        # every column reset to uniform: both right-hand sides exactly zero, the r solve warm-started from a real gradient
        fields.append([np.full(n, 300.0) for _ in range(nv)])
        flat = run(be, 2)
        its = be.last_flux_iters[0].copy()
        res = [fo.solve(M, dinv, np.zeros(n), second[0, 1, j], rtol) for j in range(nv)]
        print(f"FLUX batched, uniform state: flux_iters {its.tolist()}, restated r counts under the bn2 = 0 rule {[r['count'] for r in res]}")
        assert not any(single_rhs(single, fields[2][0])[q].any() for q in (0, 1))
        assert its[0] == 0 and (any(po.near_cut(r) for r in res) or its[1] == max(r["count"] for r in res)) and its[1] > 0
        assert not flat.any()
        be.batch_end()


# ----------------------------------------------------------------------------------------------------------------------
# h. a repeated set-up inside an open batch
# ----------------------------------------------------------------------------------------------------------------------
def test_flux_setup_repeated_inside_an_open_batch(hip):
    """hf_flux_setup allocates M1 and D^-1 anew; the batch's projection state must follow them (ensure_batch_flux sets its operator
    pointers on every call).  The projected samples of the next step are bit for bit those of a context that set up once."""
    c = case_of("fixture")
    nodes = np.arange(0, c["O"].n, 7, dtype=np.int32)
    out = []
    for repeat in (False, True):
        with step_context(hip, c) as be:
            g = open_batch(hip, be, c, 4)
            be.batch_run(g[:1], 1e-10, 0.0, 20000, None, flux_nodes=nodes, flux_components=3, flux_rtol=1e-10)
            if repeat:
                be.flux_setup()
            _, _, flux = be.batch_run(g[1:2], 1e-10, 0.0, 20000, None, flux_nodes=nodes, flux_components=3, flux_rtol=1e-10)
            out.append((flux, be.last_flux_iters.copy()))
            be.batch_end()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert np.abs(out[0][0]).max() > 0
