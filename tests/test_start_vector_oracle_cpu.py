"""The restatement of the projected start vector (tests/start_vector_oracle.py) is judged here, on the CPU, before the device is
judged against it (tests/test_gpu_start_vector.py).

A float64 trajectory on the fixture mesh of tests/golden/with_diamond_tiny.npz (1960 nodes, heated line time-varying, one sparse
direct solve per step) is replayed through the restated ring, Gram matrix, small solve and combination.  Because the stored
solutions are exact, the projection's defining properties hold to rounding.  Then the replay is repeated with one fault
injected at the probed step, and each fault must move the metrics the GPU tests assert.

Mutation table (fixture inputs of start_vector_oracle.fixture_case, probe at step PROJ_MH + 2 = 8; printed by
test_each_mutation_moves_the_metrics_meant_to_catch_it).  dots: max |G - V.F| / sum |V F| over the entries; energy: (E(alpha) -
E(alpha_ref)) / |E(alpha_ref)| on the correct G; residual: |b - A v0| over the same norm without the fault; combine: max |v0 - sum
alpha V| over the derived elementwise bound; V: the stored vector equals the state with zeroed Dirichlet rows.

  mutation                               dots      energy     residual   combine   V        caught by
  (none)                                 1.6e-16   < 1e-13    1          0         equal
  Gram column one step stale             1.0e+00   1.6e+11    1.7e+08    -         equal    dots, energy, end to end
  two slots swapped in coefficient read  -         -          5.1e+02    3.8e+15   equal    combine, end to end
  response column left at zero           1.0e+00   7.5e-08    1.13       -         equal    dots (and the weak energy shift)
  Dirichlet rows of one V not zeroed     -         -          1.35       -         differs  the exact comparison of V

Mutation floors for the two measured GPU bounds: energy 7.5e-08 (the smallest shift of a fault that moves it), end-to-end residual
ratio 5.1e+02 (the smallest among the faults that only this metric or the combine check sees; a zeroed response column and
unzeroed Dirichlet rows move it by 1.13 and 1.35 only, which no measured bound can separate from 1 - they are caught by the dots
check and by the exact comparison of V)."""
import numpy as np
import pytest

import start_vector_oracle as so

LD = np.longdouble


@pytest.fixture(scope="module")
def sizes():
    from heatflow_amd import hip_backend

    return hip_backend.projection_sizes()


@pytest.fixture(scope="module")
def traj(sizes):
    """Exact trajectory of 2 PROJ_MH + 3 steps (one LU for all, checked once against spsolve): operators, boundary values, states u[0..nsteps], right-hand sides b[1..nsteps]."""
    import scipy.sparse.linalg as spla

    mh, _ = sizes
    nsteps = 2 * mh + 3
    case = so.fixture_case(nsteps)
    op = so.Operators(case["coords"], case["tris"], case["tags"], case["tk"], case["trc"], case["dt"], case["dofs"])
    lu = spla.splu(op.Ahat.tocsc())
    u, b = [case["u0"]], [None]
    for s in range(1, nsteps + 1):
        rhs, _ = so.rhs_of_step(op, u[-1], case["g_all"][s - 1])
        u.append(lu.solve(rhs))
        b.append(rhs)
    assert np.abs(spla.spsolve(op.Ahat.tocsc(), b[3]) - u[3]).max() <= 1e-9 * np.abs(u[3]).max()
    return {"case": case, "op": op, "lu": lu, "u": u, "b": b, "nsteps": nsteps}


def replay(traj, sizes, probe, mutation=None):
    """The restated algorithm on the exact trajectory up to the start vector of step `probe`, optionally with one fault.
    Returns the quantities the GPU tests look at."""
    mh, mt = sizes
    case, op, u, b = traj["case"], traj["op"], traj["u"], traj["b"]
    dofs = case["dofs"]
    R, resp = so.RingModel(mh, mt), so.ResponseModel()
    V, F = np.zeros((mt, op.n)), np.zeros((mt, op.n))
    G = np.zeros((mt, mt))

    def column(slot, stale=False):
        for k in R.active():
            Vk, Fs = V[k], F[slot]
            if stale:                                   # the column is taken against the pair stored one step earlier
                q = (slot - 1) % mh
                Fs, Vk = F[q], (V[q] if k == slot else V[k])
            G[k, slot] = G[slot, k] = float(np.dot(Vk.astype(LD), Fs.astype(LD)))

    for s in range(1, probe + 1):
        last = s == probe
        _, new = resp.step(case["g_all"][s - 1])
        if new is not None:
            slot = mh + R.nresp
            rhs, _ = so.response_rhs(op, new)
            w = traj["lu"].solve(rhs)
            V[slot], F[slot] = so.zero_rows(w, dofs), rhs
            R.new_response()
            if not (mutation == "response_zero" and slot == mh):
                column(slot)
        pend = R.pending
        act = R.begin_step()
        if act and pend >= 0:
            column(pend, stale=(mutation == "stale_column" and last))
        if last:
            break
        slot = R.next
        V[slot], F[slot] = so.zero_rows(u[s], dofs), b[s]
        if mutation == "dirichlet_kept" and s == probe - 1:
            V[slot] = u[s].copy()
        R.end_step(s)
    f, g = b[probe], case["g_all"][probe - 1]
    Vt, Ft = V[act], F[act]
    Gt, ht, Gabs, _ = so.gram_and_rhs(Vt, Ft, f)                       # what a correct device would hold for these V, F
    Ga = G[np.ix_(act, act)]
    alpha, rank, pivots, _ = so.solve_like_device(Ga, ht.astype(np.float64))
    a_comb = alpha.copy()
    if mutation == "swap_slots":
        a_comb[[0, 1]] = a_comb[[1, 0]]
    v0, mag = so.start_vector(Vt, a_comb, dofs, g)
    clean_V = np.array([so.zero_rows(v, dofs) for v in Vt])
    v_ok, mag_ok = so.start_vector(Vt, alpha, dofs, g)
    a_ref, rank_ref = so.reference_minimiser(Gt, ht)
    e_ref = so.energy(Gt, ht, a_ref)
    return {"act": act, "V": Vt, "F": Ft, "G": Ga, "G_true": Gt, "Gabs": Gabs, "h": ht, "alpha": alpha, "rank": rank,
            "pivots": pivots, "v0": v0, "f": f, "g": g, "model": R,
            "dots": float(np.max(np.abs(Ga - Gt.astype(np.float64)) / Gabs.astype(np.float64))),
            "energy_shift": float((so.energy(Gt, ht, alpha) - e_ref) / abs(e_ref)), "rank_ref": rank_ref,
            "combine": float(np.max(np.abs(v0 - v_ok)[op.free] / np.maximum((len(act) + 1) * 2.0 ** -53 * mag_ok[op.free], 1e-300))),
            "resid": float(np.linalg.norm(f - op.Ahat @ v0)), "V_clean": bool(np.array_equal(clean_V, Vt))}


def probes(sizes):
    mh, _ = sizes
    return [1, 2, 3, mh + 1, mh + 2, 2 * mh + 2]


def test_residual_of_the_start_vector_is_orthogonal_to_the_basis_and_beats_the_extrapolations(traj, sizes):
    op, u = traj["op"], traj["u"]
    for s in probes(sizes)[1:]:
        r = replay(traj, sizes, s)
        res = r["f"] - op.Ahat @ r["v0"]
        kept = [k for k in range(len(r["act"])) if r["alpha"][k] != 0.0] if r["rank"] < len(r["act"]) else range(len(r["act"]))
        for k in kept:
            rel = abs(float(np.dot(r["V"][k].astype(LD), res.astype(LD)))) / (np.linalg.norm(r["V"][k]) * np.linalg.norm(r["f"]))
            # one rounding relative to |V_k| |f|: the boundary rows dominate |f| while the residual lives on the free rows, so the
            # figures are near 1e-25 here; eps is the level the issue names and already seven decades below a swapped slot
            assert rel <= np.finfo(float).eps, (s, k, rel)
        err = lambda v: op.energy_norm2(v - u[s])
        g = r["g"]
        cands = [u[s - 1]] + ([2 * u[s - 1] - u[s - 2]] if s >= 2 else [])
        for c in cands:
            c = c.copy()
            c[op.dofs] = g
            assert err(r["v0"]) <= err(c) * (1 + 1e-9), (s, err(r["v0"]), err(c))


def test_one_vector_reproduces_the_scalar_formula(traj, sizes):
    r = replay(traj, sizes, 2)
    assert len(r["act"]) == 1 and r["rank"] == 1
    a = float(r["h"][0] / r["G_true"][0, 0])
    assert abs(r["alpha"][0] - a) <= 4 * np.finfo(float).eps * abs(a)


def test_repeated_solution_and_zero_field_are_rank_deficient():
    rng = np.random.default_rng(0)
    n, m = 400, 4
    L = rng.standard_normal((n, n)) / np.sqrt(n)
    A = L @ L.T + np.eye(n)
    V = rng.standard_normal((m, n))
    V[2] = V[0]
    F = V @ A
    f = rng.standard_normal(n)
    G, h, _, _ = so.gram_and_rhs(V, F, f)
    alpha, rank, pivots, kept = so.solve_like_device(G.astype(float), h.astype(float))
    assert rank == m - 1 and pivots[-1] < 1e-14 and (alpha[0] == 0.0) != (alpha[2] == 0.0)
    a_ref, rank_ref = so.reference_minimiser(G, h)
    assert rank_ref == m - 1
    e, e_ref = so.energy(G, h, alpha), so.energy(G, h, a_ref)
    assert abs(float((e - e_ref) / abs(e_ref))) <= 1e-12
    Z = np.zeros((3, n))
    G, h, _, _ = so.gram_and_rhs(Z, Z, f)
    alpha, rank, _, _ = so.solve_like_device(G.astype(float), h.astype(float))
    assert rank == 0 and not alpha.any()
    assert so.reference_minimiser(G, h)[1] == 0


def test_ring_model_names_what_every_gram_entry_holds(sizes):
    mh, mt = sizes
    ev = [("step", s, s in (3, 4)) for s in range(1, mh + 3)]
    snaps = so.ring_model(mh, mt, ev)
    last = snaps[-1]                                      # after step mh + 2: slot 1 was overwritten by step mh + 2, not yet in G
    assert last["pending"] == 1 and last["next"] == 2 and last["used"].sum() == mh + 2
    assert last["content"][0] == ("step", mh + 1) and last["content"][1] == ("step", mh + 2)
    assert all(last["current"][1][l] is None and last["current"][l][1] is None for l in range(mt))
    assert last["current"][0][2] == (("step", 3), ("step", mh + 1))        # V of slot 2 against the F of the newer pair, mirrored
    assert last["current"][2][0] == (("step", 3), ("step", mh + 1))
    assert last["current"][mh][0] == (("resp", 0), ("step", mh + 1)) and last["current"][mh + 1][mh] == (("resp", 0), ("resp", 1))
    after = so.ring_model(mh, mt, ev + [("set_state",)])[-1]
    assert after["used"].tolist() == [False] * mh + [True, True] + [False] * (mt - mh - 2) and after["pending"] == -1
    assert not so.ring_model(mh, mt, ev + [("assemble",)])[-1]["used"].any()


def test_no_pivot_of_a_probed_step_lies_near_the_cut(traj, sizes):
    """The GPU file asserts the rank as an equality: legitimate only while no restated pivot is within 10x of the cut."""
    for s in probes(sizes)[1:]:
        r = replay(traj, sizes, s)
        rel = np.array(r["pivots"]) / r["pivots"][0]
        assert not ((rel > so.CUT / 10) & (rel < so.CUT * 10)).any(), (s, rel)
        assert r["rank"] == r["rank_ref"], (s, r["rank"], r["rank_ref"])
        print(f"step {s}: m = {len(r['act'])}, rank = {r['rank']}, pivots / first = {np.array2string(rel, precision=2)}")


def test_each_mutation_moves_the_metrics_meant_to_catch_it(traj, sizes):
    mh, _ = sizes
    s = mh + 2
    base = replay(traj, sizes, s)
    assert base["dots"] <= 1e-12 and abs(base["energy_shift"]) <= 1e-13 and base["combine"] <= 1.0 and base["V_clean"]
    out = {m: replay(traj, sizes, s, m) for m in ("stale_column", "swap_slots", "response_zero", "dirichlet_kept")}
    for m, r in out.items():
        print(f"{m:16s} dots {r['dots']:.2e}  energy shift {r['energy_shift']:.2e}  residual ratio {r['resid'] / base['resid']:.2e}  "
              f"combine {r['combine']:.2e}  V clean {r['V_clean']}")
    floor_e, floor_r = 7e-8, 500.0                 # the floors of the module docstring's table
    for m in ("stale_column", "response_zero"):
        assert out[m]["dots"] >= 0.9, m                                    # GPU bound: 2 gamma_d, below 1e-13
        assert out[m]["energy_shift"] >= floor_e, m
    assert out["stale_column"]["resid"] >= floor_r * base["resid"]
    assert not out["dirichlet_kept"]["V_clean"]
    assert out["swap_slots"]["combine"] >= 1e6 and out["swap_slots"]["resid"] >= floor_r * base["resid"]
