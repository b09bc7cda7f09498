"""The restatement of the read-flux projection (tests/flux_oracle.py) judged without a device, before tests/test_gpu_flux.py
holds the kernels to it: (a) it equals oracle.heat_oracle.GradientProjector, (b) the closed form - a linear field's gradient lies in
P1, so its projection is that constant vector at every node, (c) its float64 evaluations stay within 1e-15 S of the longdouble one,
a hundred times below the 1e-13 S the device is held to, (d) the spectrum of D^-1 M1, which the device's closed-form bound uses.
Then every fault of flux_oracle.MUTATIONS is injected and must be seen by the metric meant to see it; the table is printed
(pytest -s) with each fault's size as a multiple of the bound."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import flux_oracle as fo
import pcg_oracle as po

CLOSED_TOL = 1e-10
MESHES = ("jitter40", "flipped40", "l134")
_cache = {}


def mesh(name):
    if name not in _cache:
        if name == "l134":
            from test_gpu_parity import _unit_square_mesh

            coords, tris = _unit_square_mesh(*po.MESHES["l134"])
        elif name == "fixture":
            import start_vector_oracle as so

            case = so.fixture_case(1)
            coords, tris = case["coords"], case["tris"]
        elif name == "fan":
            coords, tris = fo.with_fan(*fo.jittered_lattice(40, 40, flipped=True))
        else:
            coords, tris = fo.jittered_lattice(40, 40, flipped=name == "flipped40")
        O = fo.FluxOracle(coords, tris)
        M, dinv = O.mass()
        _cache[name] = (O, spla.splu(M.tocsc()))
    return _cache[name]


def smooth_field(coords):
    """What a few heated steps leave: a hot spot on the axis on the 300 K background."""
    z, r = coords[:, 0], coords[:, 1]
    return 300.0 + 900.0 * np.exp(-((z - 0.5e-6) ** 2 + r ** 2) / (0.3e-6) ** 2)


def states(coords):
    return {"linear": fo.linear_field(coords), "rough": fo.rough_field(coords), "smooth": smooth_field(coords)}


def closed_form_error(lu, bz, br, coef=fo.LIN):
    gz, gr = lu.solve(bz), lu.solve(br)
    return max(np.abs(gz - coef[1]).max(), np.abs(gr - coef[2]).max()) / max(abs(coef[1]), abs(coef[2]))


@pytest.mark.parametrize("name", MESHES)
def test_restatement_equals_the_gradient_projector(name):
    from oracle import heat_oracle as ho

    O, lu = mesh(name)
    proj = ho.GradientProjector(O.coords, O.tris)
    M, dinv = O.mass()
    assert np.array_equal(M.indices, proj.M1.indices) and np.array_equal(M.indptr, proj.M1.indptr)
    rowmax = np.maximum.reduceat(np.abs(M.data), M.indptr[:-1])
    assert (np.abs(M.data - proj.M1.data) / np.repeat(rowmax, np.diff(M.indptr))).max() <= 1e-14
    assert abs(M - M.T).max() == 0.0
    for label, u in states(O.coords).items():
        bz, br, Sz, Sr = O.rhs(u)
        ue = u[O.tris]
        pz = np.bincount(O.flat, weights=((ue * proj.bz).sum(axis=1)[:, None] * proj.w).ravel(), minlength=O.n)
        pr = np.bincount(O.flat, weights=((ue * proj.br).sum(axis=1)[:, None] * proj.w).ravel(), minlength=O.n)
        qz, qr = fo.row_ratio(pz, bz, Sz), fo.row_ratio(pr, br, Sr)
        g = proj.project(u)
        mine = np.column_stack([lu.solve(bz), lu.solve(br)])
        rel = np.abs(mine - g).max() / np.abs(g).max()
        print(f"{name} {label}: b against GradientProjector {max(qz, qr):.1e} S, gradient {rel:.1e} of its largest entry")
        assert max(qz, qr) <= 1e-14 and rel <= 1e-10


@pytest.mark.parametrize("name", MESHES)
def test_closed_form_of_a_linear_field(name):
    O, lu = mesh(name)
    bz, br, _, _ = O.rhs(fo.linear_field(O.coords))
    err = closed_form_error(lu, bz, br)
    print(f"{name}: projection of the linear field against (c_z, c_r): {err:.1e} relative")
    assert err <= CLOSED_TOL


@pytest.mark.parametrize("name", MESHES)
def test_float64_evaluations_stay_within_the_longdouble_one(name):
    O, _ = mesh(name)
    worst, cancel = 0.0, 0.0
    for label, u in states(O.coords).items():
        bz, br, Sz, Sr = O.rhs(u)
        if label == "linear":            # b_z = c_z sum_e w there, every row well away from zero
            cancel = float(np.max(Sz / np.abs(bz)))
        for v in fo.VARIANTS:
            vz, vr, vSz, vSr = O.rhs(u, v)
            worst = max(worst, fo.row_ratio(vz, bz, Sz), fo.row_ratio(vr, br, Sr))
            assert np.allclose(vSz, Sz, rtol=1e-12, atol=0) and np.allclose(vSr, Sr, rtol=1e-12, atol=0)
    print(f"{name}: float64 evaluations within {worst:.1e} S of longdouble (bound {fo.SELF_TOL:.0e}; cancellation S/|b| up to {cancel:.1e})")
    assert worst <= fo.SELF_TOL


@pytest.mark.parametrize("name", MESHES + ("fixture", "fan"))          # every mesh tests/test_gpu_flux.py takes lambda_min of
def test_spectrum_of_the_jacobi_scaled_mass_matrix(name):
    O, _ = mesh(name)
    lo, hi = O.spectrum()
    print(f"{name}: spectrum of D^-1 M1 in [{lo:.4f}, {hi:.4f}]")
    assert 0.49 <= lo and hi <= 2.01


# ----------------------------------------------------------------------------------------------------------------------
# mutations
# ----------------------------------------------------------------------------------------------------------------------
def _columns(coords, nv=4):
    """Linear fields that differ per column: (c_z, c_r) scaled by 1 + j and turned."""
    return [(300.0 + 10.0 * j, fo.LIN[1] * (1 + j), fo.LIN[2] * (1.0 - 0.4 * j)) for j in range(nv)]


def test_every_fault_is_seen_by_the_metric_meant_to_see_it():
    O, lu = mesh("flipped40")
    M, dinv = O.mass()
    n = O.n
    u_lin = fo.linear_field(O.coords)
    bz, br, Sz, Sr = O.rhs(u_lin)
    table = []
    # faults of a single right-hand side: the row bound and the closed form
    for mut in ("weight_plain_mean", "no_fabs", "components_exchanged"):
        mz, mr, _, _ = O.rhs(u_lin, mutation=mut)
        row = max(fo.row_ratio(mz, bz, Sz), fo.row_ratio(mr, br, Sr)) / fo.ROW_TOL
        closed = closed_form_error(lu, mz, mr) / CLOSED_TOL
        table.append((mut, {"row": row, "closed": closed}, ("row", "closed")))
    # faults of the batched path: columns that differ
    cols = _columns(O.coords)
    fields = [fo.linear_field(O.coords, c) for c in cols]
    rhs = [O.rhs(u) for u in fields]
    row = max(max(fo.row_ratio(rhs[(j + 1) % len(cols)][0], rhs[j][0], rhs[j][2]), fo.row_ratio(rhs[(j + 1) % len(cols)][1], rhs[j][1], rhs[j][3]))
              for j in range(len(cols) - 1)) / fo.ROW_TOL
    closed = max(closed_form_error(lu, rhs[j + 1][0], rhs[j + 1][1], cols[j]) for j in range(len(cols) - 1)) / CLOSED_TOL
    table.append(("state_of_next_column", {"row": row, "closed": closed}, ("row",)))
    out = np.stack([np.stack([lu.solve(r[c]) for r in rhs]) for c in (0, 1)])                 # [component][column][node]
    wrong = np.ascontiguousarray(out.transpose(0, 2, 1)).reshape(out.shape)                    # written [node][column], read as above
    right = max(np.abs(out[c, j] - cols[j][1 + c]).max() / max(abs(cols[j][1]), abs(cols[j][2])) for c in (0, 1) for j in range(len(cols)))
    closed = max(np.abs(wrong[c, j] - cols[j][1 + c]).max() / max(abs(cols[j][1]), abs(cols[j][2])) for c in (0, 1) for j in range(len(cols)))
    assert right <= CLOSED_TOL
    table.append(("node_major_output", {"closed": closed / CLOSED_TOL}, ("closed",)))
    # the warm start: three consecutive projections of a field that changes; nothing but the count can see it
    steps = [O.rhs(fo.rough_field(O.coords) + 40.0 * s * smooth_field(O.coords) / 900.0)[:2] for s in range(3)]
    for rtol in (1e-6, 1e-10):
        good = fo.sequence(M, dinv, steps, rtol)
        bad = fo.sequence(M, dinv, steps, rtol, mutation="warm_start_of_z")
        cg = [r["count"] for pair in good for r in pair]
        cb = [r["count"] for pair in bad for r in pair]
        assert all(po.near_cut(r) == [] for pair in good for r in pair), "a tested residual of the restatement lies in the band"
        scale = max(np.abs(fo.final(r)).max() for pair in good for r in pair)
        drift = max(np.abs(fo.final(a) - fo.final(b)).max() for pg, pb in zip(good, bad) for a, b in zip(pg, pb)) / scale
        table.append((f"warm_start_of_z rtol {rtol:.0e}", {"count": float(sum(a != b for a, b in zip(cg, cb))), "result/rtol": drift / rtol}, ("count",)))
        print(f"warm start, rtol {rtol:.0e}: counts {cg} against {cb} with the exchange left out; results differ by {drift:.1e} of the gradient")
    print("\nfault                           seen by (size as a multiple of the bound; count: solves whose count changes)")
    for mut, seen, must in table:
        print(f"  {mut:30s} " + "  ".join(f"{k} {v:.3g}" for k, v in seen.items()) + f"   must be seen by: {', '.join(must)}")
        for k in must:
            assert seen[k] > (0 if k == "count" else 1.0), (mut, k, seen)
    assert {t[0].split()[0] for t in table} == set(fo.MUTATIONS)
