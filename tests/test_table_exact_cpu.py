"""The exact table reference (tests/table_exact.py) judged before the GPU test uses it: the coverage of the designed states from
the reference alone, float64 replicas of ktab_eval / ktab_mean inside the derived rounding model, the older float64 restatements
measured against exact values, and nine injected faults.

Measured here (worst replica error / model over the designed pairs, the designed mesh's element pairs and 1e5 random pairs per
table, a fifth of them 1e-12 .. 1 knot wide; the replica has to stay at or below 1/4):
    ktab_mean  capacity tables 3: 0.11  5: 0.14  7: 0.057  8: 0.16  11: 0.12
    ktab_eval  capacity tables 3: 0.18  5: 0.18  7: 0.11  8: 0.074  11: 0 (exact)    conductivity tables 3: 0.21  7: 0.21  11: 0  12: 0.061
Worst relative errors against the same exact values, the older restatements next to the replica (a scratch measurement before
this reference existed gave for table_mean / the replica: 51-knot bump 2.3e-15 / 1.4e-15, flat 256 knots 7.4e-14 / 2.3e-16,
random 256 knots 1.2e-13 / 3.4e-14, 256 knots with a hat 1000 x the base 4.5e-13 / 3.1e-13):
    table                              enthalpy_oracle.table_mean   ktab_mean replica   kappa_T_oracle.table_eval
    3   2 knots                        4.8e-16                      4.7e-16             1.8e-16
    5   3 knots                        4.6e-16                      3.3e-16             1.5e-16
    7   51 knots, dT 0.7               6.1e-14                      3.0e-15             5.4e-16
    8   256 knots, hat 1000 x          4.9e-13                      2.3e-13             4.4e-13
    11  5 knots, constant              1.9e-16                      3.9e-16             0
(the steep table's figures are the conditioning of s times the slope, which the model carries; table_mean is the noisier side on
the fine grid: it accumulates cum in kelvin.)
Injected faults: worst error / model on the designed set, and whether the sets of
test_gpu_enthalpy.py::test_revalued_M_and_A_are_symmetric_and_match_the_restatement see them - uniform random (u^n, e) over
150..1050 K on the small production mesh, three tags with one 51-knot grid and equal values; seen = more than 1e-13 of the value on
some triangle:
    1 one-segment branch taken below / above the table      7.9e+13   MISSED (no pair ends in the first segment from below)
    2 cum read without h.off                                5.2e+13   MISSED
    3 tail dropped when sh is an integer                    7.2e+29   MISSED
    4 int(s) without min(.., n - 2)                         no effect: both clamps return before the index is formed, in ktab_eval
                                                            and in ktab_mean, so the min cannot bind and no input shows its
                                                            absence - equal bits asserted instead of a multiple of the model
    5 midpoint replaced by Ta                               7.9e+13   seen
    6 division by Tb - Ta in kelvin                         6.3e+14   seen
    7 upper clamp at n - 2                                  9.2e+29   seen
    8 headers by position in `tags`                         inf       seen   (inf: a wrong value where the model is 0)
    9 cum built from the previous tables' values            2.5e+14   MISSED (that test never replaces tables)
Uniform random pairs on one grid miss 1, 2, 3 and 9 (and 4, which nothing can see)."""
import functools

import numpy as np
import pytest

import table_edge_cases as tc
import table_exact as tx
from table_exact import ExactTable, abs_err

FAULTS = ("one_segment_in_clamp", "cum_without_off", "tail_dropped_on_knot", "no_min", "midpoint_is_Ta", "kelvin_division",
          "clamp_at_n_minus_2", "headers_by_position", "stale_cum")
LAYOUT_FAULTS = ("headers_by_position", "stale_cum")
MISSED_BY_RANDOM_PAIRS = {"one_segment_in_clamp", "cum_without_off", "tail_dropped_on_knot", "no_min", "stale_cum"}
PREVIOUS_CV = {3: (300.0, 10.0, np.linspace(2.0e6, 2.5e6, 51)), 7: (300.0, 10.0, np.linspace(1.0e6, 3.0e6, 51))}


# ---- the device's layout and float64 replicas of its statements ---------------------------------------------------------------------
def pack(tables, order, dictionary, fault=None, previous=None):
    """(headers by dictionary slot, vals, cum) as kt_set_tables / kt_ensure_cum lay them out; a header is (t0, inv_dt, n, off)."""
    hdr = [(0.0, 0.0, 0, 0)] * len(dictionary)
    vals = []
    for pos, t in enumerate(order):
        T0, dT, v = tables[t]
        q = pos if fault == "headers_by_position" else dictionary.index(t)
        hdr[q] = (float(T0), 1.0 / float(dT), len(v), len(vals))
        vals.extend(float(x) for x in v)
    vals = np.array(vals)

    def cum_of(h, v):
        cum = np.zeros(len(v))
        for (_, _, n, off) in h:
            for i in range(1, n):
                cum[off + i] = cum[off + i - 1] + 0.5 * (v[off + i - 1] + v[off + i])
        return cum
    if fault == "stale_cum":
        ph, pv, _ = pack(previous, sorted(previous), dictionary)
        return hdr, vals, cum_of(ph, pv)
    return hdr, vals, cum_of(hdr, vals)


def _take(a, i):
    return np.take(a, i, mode="clip")                    # (lanes a branch does not select, and a fault's stray reads)


def replica_eval(h, vals, T, fault=None):
    """ktab_eval, statement for statement in float64."""
    t0, inv_dt, n, off = h
    T = np.asarray(T, dtype=np.float64)
    s = (T - t0) * inv_dt
    top = float(n - 2 if fault == "clamp_at_n_minus_2" else n - 1)
    i = np.trunc(np.clip(s, 0.0, float(n))).astype(np.int64)
    if fault != "no_min":
        i = np.minimum(i, n - 2)
    a, b = _take(vals, off + i), _take(vals, off + i + 1)
    mid = a + (s - i.astype(np.float64)) * (b - a)
    return np.where(~(s > 0.0), vals[off], np.where(s >= top, vals[off + n - 1], mid))


def replica_mean(h, vals, cum, Ta, Tb, fault=None):
    """ktab_mean, statement for statement in float64 (knot units, inv_dt = 1 / dT, the host's cum)."""
    t0, inv_dt, n, off = h
    coff = 0 if fault == "cum_without_off" else off
    Ta, Tb = np.asarray(Ta, dtype=np.float64), np.asarray(Tb, dtype=np.float64)
    lo, hi = np.minimum(Ta, Tb), np.maximum(Ta, Tb)
    sl, sh = (lo - t0) * inv_dt, (hi - t0) * inv_dt
    top = float(n - 2 if fault == "clamp_at_n_minus_2" else n - 1)
    all_low, all_high = ~(sh > 0.0), sl >= top
    below, above = ~(sl > 0.0), sh >= top

    def seg(s):
        i = np.trunc(np.clip(s, 0.0, float(n))).astype(np.int64)
        return i if fault == "no_min" else np.minimum(i, n - 2)
    il = np.where(below, 0, seg(sl))
    ih = np.where(above, n - 1, seg(sh))
    one = (il == ih) if fault == "one_segment_in_clamp" else (~below & ~above & (il == ih))
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = _take(vals, off + il), _take(vals, off + il + 1)
        sm = sl if fault == "midpoint_is_Ta" else sl + 0.5 * (sh - sl)
        mid = a + (sm - il.astype(np.float64)) * (b - a)
        x = sl - il.astype(np.float64)
        head = np.where(below, (0.0 - sl) * vals[off], (1.0 - x) * (a + (0.5 * (x + 1.0)) * (b - a)))
        jl = np.where(below, 0, il + 1)
        a, b = _take(vals, off + ih), _take(vals, off + ih + 1)
        x = sh - ih.astype(np.float64)
        tail = np.where(above, (sh - top) * vals[off + n - 1], x * (a + (0.5 * x) * (b - a)))
        if fault == "tail_dropped_on_knot":             # an end on a knot taken as the end of the segment before, its piece forgotten
            on = ~above & (x == 0.0) & (ih > 0)
            ih, tail = np.where(on, ih - 1, ih), np.where(on, 0.0, tail)
        den = (hi - lo) if fault == "kelvin_division" else (sh - sl)
        far = ((head + (_take(cum, coff + ih) - _take(cum, coff + jl))) + tail) / den
    return np.where(all_low, vals[off], np.where(all_high, vals[off + n - 1], np.where(one, mid, far)))


# ---- the sets --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh_pairs():
    """{tag: (Ta, Tb, T_e)} of the designed mesh and states."""
    coords, tris, tags, _ = tc.build_mesh()
    un, e = tc.build_states()
    Ta, Tb, Te = tx.element_Tw(un, coords, tris), tx.element_Tw(e, coords, tris), tx.element_T(e, tris)
    return {t: (Ta[tags == t], Tb[tags == t], Te[tags == t]) for t in tc.TAGS}


def _random_pairs(tab, count, seed):
    rng = np.random.default_rng(seed)
    lo, hi = tab.T0, tab.T0 + (tab.n - 1) * tab.dT
    Ta = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), count)
    Tb = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), count)
    narrow = rng.random(count) < 0.2                                        # a fifth of them 1e-12 .. 1 knot wide
    Tb[narrow] = Ta[narrow] + tab.dT * 10.0 ** rng.uniform(-12.0, 0.0, int(narrow.sum()))
    return Ta, Tb


def _designed(tag, tables):
    tab = ExactTable(*tables[tag])
    pairs = tc.designed_pairs(tab)
    Ta, Tb, Te = _mesh_pairs()[tag]
    if tables is tc.K_TABLES:
        pts = np.array(tc.designed_points(tab))
        return tab, np.concatenate([pts, Te]), np.concatenate([pts, Te])
    # and ends one step inside two neighbouring knots: w just under 1, where rounded ends make the device read cum[k] - cum[k-1]
    pairs = pairs + [(tc.ulps(tc.knot_float(tab, k - 1), 1), tc.ulps(tc.knot_float(tab, k), -1)) for k in tc.special_knots(tab.n) if k >= 1]
    return tab, np.concatenate([[p[0] for p in pairs], Ta]), np.concatenate([[p[1] for p in pairs], Tb])


def _worst_ratio(err, model):
    """max err / model; an error where the model is 0 (an exact return) is infinite."""
    err, model = np.asarray(err), np.asarray(model)
    r = np.where(model > 0.0, err / np.where(model > 0.0, model, 1.0), np.where(err > 0.0, np.inf, 0.0))
    return float(r.max())


def _eval_errors(tab, T, got):
    return np.array([abs_err(g, tab.value(t)) for t, g in zip(T, got)])


# ---- 1. the coverage condition, from the reference alone --------------------------------------------------------------------------
@pytest.mark.parametrize("rotate", [0, 1])
def test_every_branch_class_has_its_triangles(rotate):
    coords, tris, tags, _ = tc.build_mesh()
    assert len(coords) <= 10500 and coords[:, 1].min() == 0.0
    un, e = tc.build_states(rotate=rotate)
    Ta, Tb = tx.element_Tw(un, coords, tris), tx.element_Tw(e, coords, tris)
    for t, tab in tc.exact_tables(tc.CV_TABLES).items():
        counts = tc.class_counts(tab, Ta[tags == t], Tb[tags == t])
        print("capacity table of tag", t, dict(sorted(counts.items())))
        assert not tc.missing_classes(counts, tx.pair_classes(tab)), t
        for T in (un, e):                                                  # the plain value at T_e (the lagged forms)
            assert not tc.missing_classes(tc.class_counts(tab, tx.element_T(T, tris)[tags == t]), tx.POINT_CLASSES), t
    for t, tab in tc.exact_tables(tc.K_TABLES).items():
        for T in (un, e):
            counts = tc.class_counts(tab, tx.element_T(T, tris)[tags == t])
            assert not tc.missing_classes(counts, tx.POINT_CLASSES), (t, counts)


def test_the_classifier_names_the_designed_pairs():
    tab = ExactTable(*tc.CV_TABLES[8])
    k = tc.knot_float(tab, 60)
    assert tab.classify_pair(k, k) == "equal:knot" and tab.classify_point(tc.ulps(k, 1)) == "segment"
    assert tab.classify_pair(tc.ulps(k, -1), tc.ulps(k, 1)) == "straddle_one_knot"
    assert tab.classify_pair(k, tc.ulps(k, 1)) == "one_segment+knot" and tab.classify_pair(k - 0.9, k) == "one_segment+knot"
    assert tab.classify_pair(k - 3.0, k + 3.0) == "straddle_one_knot+knot" and tab.classify_pair(k - 4.0, k + 4.0) == "span_knots"
    assert tab.classify_pair(100.0, 200.0) == "below+knot" and tab.classify_pair(150.0, 100.0) == "below"
    assert tab.classify_pair(199.0, 201.0) == "below_into_interior" and tab.classify_pair(964.0, 966.0) == "interior_into_above"
    assert tab.classify_pair(1000.0, 100.0) == "below_through_above" and tab.classify_pair(965.0, 970.0) == "above+knot"
    # the exact functions on a case done by hand: v = 1, 3 on 0, 2: the mean over [-1, 3] is (1 + 4 + 3) / 4
    t2 = ExactTable(0.0, 2.0, [1.0, 3.0])
    assert t2.mean(-1.0, 3.0) == 2 and t2.mean(3.0, -1.0) == 2 and t2.value(0.5) == 1.5 and t2.mean(0.5, 0.5) == 1.5
    assert t2.integral(0.0, 1.0) == 1.5 and t2.heat_term(0.25, 1.0, 0.0) == -0.375


# ---- 2. the replicas inside the model, the old restatements measured ----------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(tc.CV_TABLES))
def test_the_replicas_stay_inside_the_model(tag):
    from enthalpy_oracle import table_mean
    from kappa_T_oracle import table_eval

    tab, Ta, Tb = _designed(tag, tc.CV_TABLES)
    ra, rb = _random_pairs(tab, 100000, 40 + tag)
    Ta, Tb = np.concatenate([Ta, ra]), np.concatenate([Tb, rb])
    hdr, vals, cum = pack(tc.CV_TABLES, tc.CV_ORDER, tc.TAGS)
    h = hdr[tc.TAGS.index(tag)]
    exact_m = [tab.mean(a, b) for a, b in zip(Ta, Tb)]
    exact_v = [tab.value(a) for a in Ta]
    err_m = np.array([abs_err(g, x) for g, x in zip(replica_mean(h, vals, cum, Ta, Tb), exact_m)])
    err_v = np.array([abs_err(g, x) for g, x in zip(replica_eval(h, vals, Ta), exact_v)])
    r_m, r_v = _worst_ratio(err_m, tab.model_mean(Ta, Tb)), _worst_ratio(err_v, tab.model_eval(Ta))
    old_m = np.array([abs_err(g, x) for g, x in zip(table_mean(Ta, Tb, *tc.CV_TABLES[tag]), exact_m)])
    old_v = np.array([abs_err(g, x) for g, x in zip(table_eval(Ta, *tc.CV_TABLES[tag]), exact_v)])
    print(f"tag {tag}: replica / model: ktab_mean {r_m:.2g}, ktab_eval {r_v:.2g}; worst relative error: ktab_mean replica "
          f"{(err_m / np.array([float(x) for x in exact_m])).max():.2g}, table_mean {(old_m / np.array([float(x) for x in exact_m])).max():.2g}, "
          f"table_eval {(old_v / np.array([float(x) for x in exact_v])).max():.2g}")
    assert r_m <= 0.25 and r_v <= 0.25
    assert (old_m / np.array([float(x) for x in exact_m])).max() < 1e-9        # (measured, not held to the model)
    # symmetric in its arguments, bit for bit
    assert np.array_equal(replica_mean(h, vals, cum, Ta, Tb), replica_mean(h, vals, cum, Tb, Ta))


@pytest.mark.parametrize("tag", sorted(tc.K_TABLES))
def test_the_value_replica_stays_inside_the_model_on_the_conductivity_tables(tag):
    tab, T, _ = _designed(tag, tc.K_TABLES)
    T = np.concatenate([T, _random_pairs(tab, 100000, 60 + tag)[0]])
    hdr, vals, _ = pack(tc.K_TABLES, tc.K_ORDER, tc.TAGS)
    err = _eval_errors(tab, T, replica_eval(hdr[tc.TAGS.index(tag)], vals, T))
    r = _worst_ratio(err, tab.model_eval(T))
    print(f"conductivity table of tag {tag}: ktab_eval replica / model {r:.2g}")
    assert r <= 0.25


# ---- 3. injected faults -------------------------------------------------------------------------------------------------------------
def _fault_ratio(fault, tables, order, dictionary, sets, constants, previous):
    """The worst error / model of the faulty replica over {tag: (table, Ta, Tb)}, and the worst error relative to the value."""
    hdr, vals, cum = pack(tables, order, dictionary, fault if fault in LAYOUT_FAULTS else None, previous)
    worst, rel = 0.0, 0.0
    for t, (tab, Ta, Tb, exact, model) in sets.items():
        h = hdr[dictionary.index(t)]
        if h[2] == 0:                                                       # no header in the tag's slot: the constant
            got = np.full(len(Ta), constants[t])
        else:
            got = replica_mean(h, vals, cum, Ta, Tb, None if fault in LAYOUT_FAULTS else fault)
        err = np.array([abs_err(g, x) for g, x in zip(got, exact)])
        worst = max(worst, _worst_ratio(err, model))
        rel = max(rel, float((err / np.array([float(x) for x in exact])).max()))
    return worst, rel


def _with_exact(tab, Ta, Tb):
    return tab, Ta, Tb, [tab.mean(a, b) for a, b in zip(Ta, Tb)], tab.model_mean(Ta, Tb)


@functools.lru_cache(maxsize=None)
def _designed_sets():
    return {t: _with_exact(*_designed(t, tc.CV_TABLES)) for t in tc.CV_TABLES}


@functools.lru_cache(maxsize=None)
def _random_pair_sets():
    """The sets of test_gpu_enthalpy.py::test_revalued_M_and_A_are_symmetric_and_match_the_restatement: the small production mesh, the bump on the three insulator tags, one uniform
    random vector over 150..1050 K for u^n and one for e."""
    from conftest import build_case
    from enthalpy_oracle import bump_tables
    from helpers import material_tables

    cfg, stack, mesh = build_case("geballe_with_diamond", 8.0)
    _, trc = material_tables(stack, mesh)
    ct = bump_tables(trc, [mesh.material_tags[m.name] for m in stack.materials if m.name.endswith("ins")])
    rng = np.random.default_rng(7)
    n = len(mesh.coords)
    un, e = 150.0 + 900.0 * rng.random(n), 150.0 + 900.0 * rng.random(n)
    Ta, Tb = tx.element_Tw(un, mesh.coords, mesh.tris), tx.element_Tw(e, mesh.coords, mesh.tris)
    tags = np.asarray(mesh.tags)
    sets = {t: _with_exact(ExactTable(*ct[t]), Ta[tags == t], Tb[tags == t]) for t in ct}
    return ct, sorted(ct), sorted(int(t) for t in np.unique(tags)), sets, trc


@pytest.mark.parametrize("fault", FAULTS)
def test_injected_faults_exceed_the_model_a_hundredfold(fault):
    sets = _designed_sets()
    ratio, _ = _fault_ratio(fault, tc.CV_TABLES, tc.CV_ORDER, tc.TAGS, sets, tc.TAG_RC, PREVIOUS_CV)
    ct, order, dictionary, random_sets, trc = _random_pair_sets()
    previous = {t: (v[0], v[1], np.asarray(v[2]) * 1.0) for t, v in ct.items()}       # that test never replaces tables: the same ones
    _, rel = _fault_ratio(fault, ct, order, dictionary, random_sets, trc, previous)
    seen_by_random = rel > 1e-13
    print(f"{fault}: designed set {ratio:.2g} x the model; uniform random pairs on one grid {'see it' if seen_by_random else 'MISS it'} ({rel:.2g} of the value)")
    if fault == "no_min":
        # both clamps return before the index is formed, so int(s) <= n - 2 already: the min cannot bind, and no input can show
        # its absence.  Equal bits on every designed pair is all there is to assert.
        assert ratio <= 0.25 and not seen_by_random
        for t, (tab, Ta, Tb, _, _) in sets.items():
            hdr, vals, cum = pack(tc.CV_TABLES, tc.CV_ORDER, tc.TAGS)
            h = hdr[tc.TAGS.index(t)]
            assert np.array_equal(replica_mean(h, vals, cum, Ta, Tb, "no_min"), replica_mean(h, vals, cum, Ta, Tb))
        return
    assert ratio >= 100.0
    assert seen_by_random == (fault not in MISSED_BY_RANDOM_PAIRS)
