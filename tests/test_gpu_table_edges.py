"""The table evaluators on the GPU, branch by branch against exact arithmetic (tests/table_exact.py) on the designed tables, mesh
and states of tests/table_edge_cases.py: the enthalpy form's M and A entry by entry within the derived rounding model, the lagged
forms (conductivity tables, capacity tables, both, and with anisotropy multipliers), the Picard steady set-up's stiffness through
its held load, tables replaced under the enthalpy form, the batched kernel column by column, and the stored heat.  Re-valuations
and get_csr only; every worst figure is printed as a multiple of its bound.

Measured on the MI355X (one run of this file, profiles/table_edges_gpu_tests.txt), worst difference / bound: M 0.060 (the lagged
forms; 0.057 at e = u^n, 0.019 at the designed pairs), A 0.031 (with multipliers; 0.014 without), the steady stiffness through the
held load 0.0016, the stored heat 0.0010; every bit comparison equal."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

import table_edge_cases as tc
import table_exact as tx
from helpers import csr_values_on_pattern

pytestmark = pytest.mark.gpu

GEOMETRY = 1e-13            # of the summands of an entry: the project's figure for the float64 geometry
ANISO = {3: (2.0, 0.5), 7: (0.25, 3.0), 2: (1.5, 1.0)}      # (m_r, m_z); tags 3 and 7 carry both kinds of table, tag 2 none


@functools.lru_cache(maxsize=None)
def _mesh():
    from oracle import heat_oracle as ho

    coords, tris, tags, bc = tc.build_mesh()
    one = np.ones(len(tris))
    Me1, Ke1 = ho.element_matrices(coords, tris.astype(np.int64), one, one)
    return coords, tris, tags, bc, Me1, Ke1


@functools.lru_cache(maxsize=None)
def _states():
    """Eight designed states (four (u^n, e) pairs); read-only."""
    out = []
    for rot in range(4):
        out.extend(tc.build_states(seed=9 + rot, rotate=rot))
    for s in out:
        s.setflags(write=False)
    return tuple(out)


def _constants(table):
    _, _, tags, *_ = _mesh()
    return np.array([float(table[int(t)]) for t in tags])


def _exact_values(tables, constants, T):
    """(coefficient as float64, model / coefficient) per element: the table's exact value at T for a tabled tag."""
    _, _, tags, *_ = _mesh()
    c, rel = _constants(constants), np.zeros(len(tags))
    for t, tab in tc.exact_tables(tables).items():
        sel = np.nonzero(tags == t)[0]
        c[sel] = [float(tab.value(x)) for x in T[sel]]
        rel[sel] = tab.model_eval(T[sel]) / c[sel] + tx.U                    # (+ the reference's own rounding to float64)
    return c, rel


def _exact_means(tables, constants, Ta, Tb):
    _, _, tags, *_ = _mesh()
    c, rel = _constants(constants), np.zeros(len(tags))
    for t, tab in tc.exact_tables(tables).items():
        sel = np.nonzero(tags == t)[0]
        c[sel] = [float(tab.mean(a, b)) for a, b in zip(Ta[sel], Tb[sel])]
        rel[sel] = tab.model_mean(Ta[sel], Tb[sel]) / c[sel] + tx.U
    return c, rel


def _assemble(Ae):
    from oracle import heat_oracle as ho

    coords, tris, *_ = _mesh()
    return ho.assemble_csr(len(coords), tris.astype(np.int64), Ae)


def _reference(c, c_rel, k, k_rel, dt, Ke1=None):
    """(M, A not eliminated, bound on M, bound on A) from per-element coefficients and their relative models."""
    _, _, _, _, Me1, Ke1_iso = _mesh()
    Ke1 = Ke1_iso if Ke1 is None else Ke1
    w = lambda a: a[:, None, None]
    M, A = _assemble(Me1 * w(c)), _assemble(Me1 * w(c) + dt * (Ke1 * w(k)))
    bM = _assemble(np.abs(Me1) * w(c * (c_rel + GEOMETRY)))
    bA = _assemble(np.abs(Me1) * w(c * (c_rel + GEOMETRY)) + dt * (np.abs(Ke1) * w(k * (k_rel + GEOMETRY))))
    return M, A, bM, bA


def _held_to(label, got, ref, bound, rowptr, colidx):
    """Assert |got - ref| <= bound entry by entry; returns and prints the worst multiple of the bound."""
    r, b = csr_values_on_pattern(ref, rowptr, colidx), csr_values_on_pattern(bound, rowptr, colidx)
    err = np.abs(got - r)
    ratio = np.where(b > 0.0, err / np.where(b > 0.0, b, 1.0), np.where(err > 0.0, np.inf, 0.0))
    rel = (err / np.maximum(np.abs(r), 1e-300))[r != 0.0].max()
    print(f"{label}: worst difference {ratio.max():.3g} x its bound ({rel:.2e} of the entry at worst)")
    assert ratio.max() <= 1.0, label
    return float(ratio.max())


def _symmetric(vals, rowptr, colidx):
    n = len(rowptr) - 1
    S = sp.csr_matrix((vals, colidx, rowptr), shape=(n, n))
    return (S != S.T).nnz == 0


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _set_tables(hip, be, kind, tables, order):
    """hf_set_kappa_tables / hf_set_rhoc_tables with the tables in the order given (the wrapper sorts by tag: not wanted here)."""
    order = [t for t in order if t in tables]
    assert order != sorted(order)
    tags = hip._i32(order)
    t0, dT = hip._f64([tables[t][0] for t in order]), hip._f64([tables[t][1] for t in order])
    nk = hip._i32([len(tables[t][2]) for t in order])
    vals = hip._f64(np.concatenate([np.asarray(tables[t][2], dtype=np.float64) for t in order]))
    args = (be._ctx, len(order), hip._pi(tags), hip._pd(t0), hip._pd(dT), hip._pi(nk), hip._pd(vals))
    be._check(be._lib.hf_set_kappa_tables(*args, 1) if kind == "kappa" else be._lib.hf_set_rhoc_tables(*args))


def _context(hip, state, dt, kt=None, cv=None, form="lagged", aniso=None):
    coords, tris, tags, bc, *_ = _mesh()
    be = hip.HeatflowHIP(0)
    try:
        be.set_mesh(coords, tris, tags)
        be.set_materials(tc.TAGS, [tc.TAG_K[t] for t in tc.TAGS], [tc.TAG_RC[t] for t in tc.TAGS])
        if aniso:
            be.set_aniso_tables(True)
            be.set_anisotropy(aniso)
        be.set_dirichlet(bc)
        be.set_precond(0)
        if kt:
            _set_tables(hip, be, "kappa", kt, tc.K_ORDER)
        if cv:
            _set_tables(hip, be, "rhoc", cv, tc.CV_ORDER)
        if form == "enthalpy":
            be.set_capacity_form("enthalpy")
        be.set_state(state)
        be.assemble(dt, hip.ASM_ROW_GATHER)
    except BaseException:
        be.close()
        raise
    return be


@functools.lru_cache(maxsize=None)
def _dt_and_selection():
    """(dt, rows, columns): the step at which dt |K_ij| >= 100 |M_ij| on the selected off-diagonals, so that a slip in kappa is not
    hidden under M.  From the largest capacities and the smallest conductivities of every tag; selected are the off-diagonals
    whose K_ij is not one of a jittered right triangle's near-orthogonal pairs (|K_ij| >= 5 % of the row's diagonal), where K_ij
    can be as close to 0 as the jitter makes it."""
    _, _, tags, _, Me1, Ke1 = _mesh()
    c_hi = np.array([max(tc.TAG_RC[int(t)], np.max(tc.CV_TABLES[int(t)][2]) if int(t) in tc.CV_TABLES else 0.0) for t in tags])
    k_lo = np.array([min(tc.TAG_K[int(t)], np.min(tc.K_TABLES[int(t)][2]) if int(t) in tc.K_TABLES else np.inf) for t in tags])
    M, K = _assemble(np.abs(Me1) * c_hi[:, None, None]).tocoo(), _assemble(Ke1 * k_lo[:, None, None]).tocsr()
    Kij = np.abs(np.asarray(K[M.row, M.col]).ravel())
    off = (M.row != M.col) & (Kij >= 0.05 * K.diagonal()[M.row])
    return float(100.0 * (M.data[off] / Kij[off]).max()), M.row[off], M.col[off]


def _dt():
    return _dt_and_selection()[0]


def _check_point_coverage(tables, T):
    _, _, tags, *_ = _mesh()
    for t, tab in tc.exact_tables(tables).items():
        counts = tc.class_counts(tab, T[tags == t])
        assert not tc.missing_classes(counts, tx.POINT_CLASSES), (t, counts)


# ---- 1. the enthalpy form -----------------------------------------------------------------------------------------------------------
def test_enthalpy_form_matches_the_exact_chord_capacities(hip):
    from oracle import heat_oracle as ho

    coords, tris, tags, bc, *_ = _mesh()
    un, e = _states()[:2]
    dt = _dt()
    Ta, Tb, Te = tx.element_Tw(un, coords, tris), tx.element_Tw(e, coords, tris), tx.element_T(e, tris)
    for t, tab in tc.exact_tables(tc.CV_TABLES).items():                      # the coverage condition, from the reference alone
        assert not tc.missing_classes(tc.class_counts(tab, Ta[tags == t], Tb[tags == t]), tx.pair_classes(tab)), t
    _check_point_coverage(tc.K_TABLES, Te)
    _check_point_coverage(tc.CV_TABLES, Ta)
    be = _context(hip, un, dt, kt=tc.K_TABLES, cv=tc.CV_TABLES, form="enthalpy")
    try:
        be.enthalpy_revalue(un, e)
        rowptr, colidx, A, M = be.get_csr()
        be.enthalpy_revalue(e, un)
        M_swapped = be.get_csr()[3]
        be.enthalpy_revalue(un, un)
        _, _, A_same, M_same = be.get_csr()
    finally:
        be.close()
    k, k_rel = _exact_values(tc.K_TABLES, tc.TAG_K, Te)
    c, c_rel = _exact_means(tc.CV_TABLES, tc.TAG_RC, Ta, Tb)
    M_ref, A_ref, bM, bA = _reference(c, c_rel, k, k_rel, dt)
    _held_to("enthalpy form, M at (u^n, e)", M, M_ref, bM, rowptr, colidx)
    _held_to("enthalpy form, A at (u^n, e)", A, ho.eliminate_dirichlet(A_ref, bc), bA, rowptr, colidx)
    assert _symmetric(M, rowptr, colidx) and _symmetric(A, rowptr, colidx)
    assert _same_bits(M, M_swapped)                                            # the chord is symmetric in its ends, bit for bit
    # e = u^n: the table's value at Tw_e(u^n), conductivities at T_e(u^n)
    k, k_rel = _exact_values(tc.K_TABLES, tc.TAG_K, tx.element_T(un, tris))
    c, c_rel = _exact_values(tc.CV_TABLES, tc.TAG_RC, Ta)
    M_ref, A_ref, bM, bA = _reference(c, c_rel, k, k_rel, dt)
    _held_to("enthalpy form, M at (u^n, u^n)", M_same, M_ref, bM, rowptr, colidx)
    _held_to("enthalpy form, A at (u^n, u^n)", A_same, ho.eliminate_dirichlet(A_ref, bc), bA, rowptr, colidx)
    assert _symmetric(M_same, rowptr, colidx) and _symmetric(A_same, rowptr, colidx)
    assert (np.abs(M - M_same) / np.abs(M_same)).max() > 0.01                  # the pair matters


# ---- 2. the lagged forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", ["k", "cv", "both", "both+aniso"])
def test_lagged_forms_match_the_exact_table_values(hip, kinds):
    from aniso_oracle import cell_multipliers, element_matrices_aniso
    from oracle import heat_oracle as ho

    coords, tris, tags, bc, _, Ke1 = _mesh()
    u = _states()[1]
    dt = _dt()
    kt = tc.K_TABLES if kinds != "cv" else {}
    cv = tc.CV_TABLES if kinds != "k" else {}
    aniso = ANISO if kinds.endswith("aniso") else None
    Te = tx.element_T(u, tris)
    _check_point_coverage(kt, Te)                                              # (on the lattice with multipliers too)
    _check_point_coverage(cv, Te)
    be = _context(hip, u, dt, kt=kt, cv=cv, aniso=aniso)                       # hf_assemble values the operators at the state
    try:
        rowptr, colidx, A, M = be.get_csr()
    finally:
        be.close()
    if aniso:
        m_r, m_z = cell_multipliers(tags, aniso)
        _, Ke1 = element_matrices_aniso(coords, tris.astype(np.int64), np.ones(len(tris)), np.ones(len(tris)), m_r, m_z)
    k, k_rel = _exact_values(kt, tc.TAG_K, Te)
    c, c_rel = _exact_values(cv, tc.TAG_RC, Te)
    M_ref, A_ref, bM, bA = _reference(c, c_rel, k, k_rel, dt, Ke1)
    _held_to(f"lagged {kinds}, M", M, M_ref, bM, rowptr, colidx)
    _held_to(f"lagged {kinds}, A", A, ho.eliminate_dirichlet(A_ref, bc), bA, rowptr, colidx)
    assert _symmetric(M, rowptr, colidx) and _symmetric(A, rowptr, colidx)
    # dt |K_ij| >= 100 |M_ij| on every off-diagonal _dt_and_selection chose (isotropic: the multipliers move K_ij entry by entry)
    _, rows, cols = _dt_and_selection()
    Ms, Ks = np.abs(np.asarray(M_ref[rows, cols]).ravel()), np.abs(np.asarray((A_ref - M_ref)[rows, cols]).ravel())
    Mo = csr_values_on_pattern(M_ref, rowptr, colidx)
    off = (np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)) != colidx) & (Mo != 0.0)
    share = float(np.mean(np.abs(csr_values_on_pattern(A_ref, rowptr, colidx) - Mo)[off] >= 100.0 * np.abs(Mo[off])))
    print(f"lagged {kinds}: dt = {dt:.3g} s, dt |K_ij| / |M_ij| >= {(Ks / Ms).min():.3g} on the {len(rows)} selected off-diagonals, "
          f">= 100 on {100.0 * share:.2f} % of all {int(off.sum())}")
    if not aniso:
        assert np.all(Ks >= 100.0 * Ms)
    assert share >= 0.99


def test_picard_steady_stiffness_matches_the_exact_table_values(hip):
    """hf_steady_picard_setup values K at the state u through the conductivity tables; hf_hold_load hands (K v)_i out on the rows
    off the transient's Dirichlet set for the state v of that moment (the window of test_gpu_steady_picard.py).  v is a random
    vector without patches, set after the set-up: inside a patch of u itself K_e u_e = 0, and the designed triangles would not
    show in K(u) u."""
    coords, tris, tags, bc, _, Ke1 = _mesh()
    u = _states()[1]
    v = np.random.default_rng(31).uniform(250.0, 900.0, len(u))
    Te = tx.element_T(u, tris)
    _check_point_coverage(tc.K_TABLES, Te)
    steady = np.arange(0, len(coords), 97, dtype=np.int32)
    be = _context(hip, u, _dt(), kt=tc.K_TABLES)
    try:
        be.steady_picard_setup(steady, 0)
        be.set_state(v)
        be.hold_load()
        F = be.get_load()
    finally:
        be.close()
    k, k_rel = _exact_values(tc.K_TABLES, tc.TAG_K, Te)
    K = _assemble(Ke1 * k[:, None, None])
    bK = _assemble(np.abs(Ke1) * (k * (k_rel + GEOMETRY))[:, None, None])
    ref, bound = K @ v, bK @ np.abs(v) + GEOMETRY * (abs(K) @ np.abs(v))        # (the product's own roundings in the second term)
    free = np.setdiff1d(np.arange(len(u)), bc)
    assert np.all(F[bc] == 0.0)
    ratio = (np.abs(F - ref)[free] / bound[free]).max()
    print(f"Picard steady stiffness through the held load: worst difference {ratio:.3g} x its bound")
    assert ratio <= 1.0
    # the load is K(u) v, not K(v) v: the tables were valued at u
    kv, _ = _exact_values(tc.K_TABLES, tc.TAG_K, tx.element_T(v, tris))
    other = _assemble(Ke1 * kv[:, None, None]) @ v
    assert (np.abs(F - other)[free] / bound[free]).max() > 1e6


# ---- 3. tables replaced under the form ----------------------------------------------------------------------------------------------
def test_replaced_tables_under_the_enthalpy_form_give_a_fresh_contexts_bits(hip):
    un, e = _states()[:2]
    dt = _dt()
    first = {3: (300.0, 10.0, np.linspace(2.0e6, 2.5e6, 51)), 7: (310.0, 5.0, np.linspace(1.0e6, 3.0e6, 33)),
             8: (250.0, 40.0, np.array([2.0e6, 2.2e6, 1.8e6]))}
    be = _context(hip, un, dt, kt=tc.K_TABLES, cv=first, form="enthalpy")
    try:
        be.enthalpy_revalue(un, e)
        M_first = be.get_csr()[3]
        _set_tables(hip, be, "rhoc", tc.CV_TABLES, tc.CV_ORDER)                 # other tags, lengths, offsets and values
        be.set_state(un)
        be.assemble(dt, hip.ASM_ROW_GATHER)
        be.enthalpy_revalue(un, e)
        _, _, A, M = be.get_csr()
    finally:
        be.close()
    fresh = _context(hip, un, dt, kt=tc.K_TABLES, cv=tc.CV_TABLES, form="enthalpy")
    try:
        fresh.enthalpy_revalue(un, e)
        _, _, A2, M2 = fresh.get_csr()
    finally:
        fresh.close()
    assert _same_bits(M, M2) and _same_bits(A, A2)
    assert not np.array_equal(M, M_first)


# ---- 4. the batched kernel ----------------------------------------------------------------------------------------------------------
def test_batched_columns_are_the_single_runs_bit_for_bit(hip):
    states = _states()
    nv, dt = len(states), _dt()
    assert nv == 8
    be = _context(hip, states[0], dt, kt=tc.K_TABLES, cv=tc.CV_TABLES)
    try:
        be.set_batch_tables(True)
        be.batch_begin(nv, 1)
        for j in range(nv):
            be.batch_set_state(j, states[j])
        be.batch_revalue()
        got = [be.batch_get_operator(j, want_M=True) for j in range(nv)]
        be.batch_end()
        rowptr, colidx = be.get_csr(values=False)[:2]
        diag = np.nonzero(np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)) == colidx)[0]
        for j in range(nv):
            be.set_state(states[j])
            be.assemble(dt, hip.ASM_ROW_GATHER)
            _, _, A, M = be.get_csr()
            assert _same_bits(got[j]["A"], A) and _same_bits(got[j]["M"], M) and _same_bits(got[j]["dinv"], 1.0 / A[diag]), j
            assert not np.array_equal(got[j]["M"], got[(j + 1) % nv]["M"])
    finally:
        be.close()


# ---- 5. the stored heat -------------------------------------------------------------------------------------------------------------
def _heat_classes(tab, T_ref):
    where = tab.classify_point(T_ref)
    if where == "below":
        return ["below", "below_into_interior", "below_through_above"]
    if where == "above":
        return ["above", "interior_into_above", "below_through_above"]
    return ["one_segment", "below_into_interior", "interior_into_above"] + ["straddle_one_knot"] * (tab.n >= 3) + ["span_knots"] * (tab.n >= 4)


def test_stored_heat_matches_the_exact_sums(hip):
    coords, tris, tags, *_ = _mesh()
    e = _states()[1]
    Tw, vol = tx.element_Tw(e, coords, tris), tx.element_volume(coords, tris)
    tabs = tc.exact_tables(tc.CV_TABLES)
    be = _context(hip, e, _dt(), cv=tc.CV_TABLES)
    try:
        out = {T_ref: (be.stored_heat(T_ref), be.stored_heat(T_ref)) for T_ref in tc.HEAT_REFS}
    finally:
        be.close()
    for T_ref, (heat, again) in out.items():
        assert _same_bits(heat, again)
        for t in tc.TAGS:
            sel = np.nonzero(tags == t)[0]
            if t in tabs:
                tab = tabs[t]
                ref = np.full(len(sel), T_ref)
                counts = tc.class_counts(tab, ref, Tw[sel])
                assert not tc.missing_classes(counts, _heat_classes(tab, T_ref)), (T_ref, t, counts)
                terms = [tab.heat_term(v, T_ref, T) for v, T in zip(vol[sel], Tw[sel])]
                cm = np.array([float(tab.mean(T_ref, T)) for T in Tw[sel]])
                rel = tab.model_mean(ref, Tw[sel]) / cm + tx.U
            else:
                terms = [Fraction(float(v)) * Fraction(tc.TAG_RC[t]) * (Fraction(float(T)) - Fraction(T_ref)) for v, T in zip(vol[sel], Tw[sel])]
                rel = np.zeros(len(sel))
            mag = np.array([abs(float(x)) for x in terms])
            bound = float((mag * (rel + GEOMETRY)).sum())
            err = abs(Fraction(float(heat[t])) - sum(terms))
            print(f"stored heat, T_ref = {T_ref} K, tag {t}: {heat[t]:.6e} J/rad, difference {float(err) / bound:.3g} x its bound "
                  f"({float(err) / mag.sum():.2e} of sum |terms|)")
            assert float(err) <= bound, (T_ref, t)
        assert np.all(heat[[q for q in range(len(heat)) if q not in tc.TAGS]] == 0.0)
