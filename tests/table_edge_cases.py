"""Designed tables, mesh and states for the branch-by-branch tests of the table evaluators (tests/test_table_exact_cpu.py,
tests/test_gpu_table_edges.py; the reference is tests/table_exact.py).  TEST CODE: never imported by heatflow_amd.

Tables: seven cell tags, none of them on the grid of the other tests (300..800 K, dT = 10, 51 knots) except one conductivity table.
    tag  2  no table
    tag  3  capacity: 2 knots (400 K, dT 300)                conductivity: 51 knots (300 K, dT 10)
    tag  5  capacity: 3 knots (250 K, dT 128)                - (a capacity table on a tag without a conductivity table)
    tag  7  capacity: 51 knots (301.3 K, dT 0.7: no knot but the first is a float64)    conductivity: 256 knots (280 K, dT 0.25)
    tag  8  capacity: 256 knots (200 K, dT 3), a hat 1000 x the base around knot 60     -
    tag 11  capacity: 5 knots, constant                       conductivity: 2 knots, constant
    tag 12  -                                                 conductivity: 7 knots (290 K, dT 12.5)
CV_ORDER and K_ORDER are the orders the tables are handed over in: neither ascending (the tag dictionary's order) nor equal.

Mesh: a lattice of 127 x 80 nodes from the axis r = 0, inner nodes jittered by 0.3 of the spacing, half the triangles clockwise,
the triangle order shuffled (the recipe of test_general_triangles_random_meshes); tags in bands along z.

States: inside each tabled band, patches of 4 x 4 nodes (pitch 4, so no two share a node) constant in u^n and in e: the 18 triangles
inside a patch have (Ta, Tb) equal to the patch's pair up to the roundings of Tw_e.  Everywhere else random values from 20 % below
each table of the tag to 20 % above.  `rotate` moves every pair to another patch of its band: other triangles, the same pairs."""

import numpy as np

from table_exact import ExactTable

UNTABLED = 2
_i51, _i256 = np.arange(51), np.arange(256)
CV_TABLES = {
    3: (400.0, 300.0, np.array([1.6e6, 3.1e6])),
    5: (250.0, 128.0, np.array([2.2e6, 1.3e6, 2.9e6])),
    7: (301.3, 0.7, 2.0e6 * (1.0 + 0.25 * np.sin(0.37 * _i51))),
    8: (200.0, 3.0, 1.9e6 * (1.0 + 1000.0 * np.maximum(0.0, 1.0 - np.abs(_i256 - 60.0) / 4.0))),
    11: (350.0, 50.0, np.full(5, 2.4e6)),
}
K_TABLES = {
    3: (300.0, 10.0, 12.0 * 300.0 / (300.0 + 10.0 * _i51)),
    7: (280.0, 0.25, 5.0 + 3.0 * np.cos(0.11 * _i256)),
    11: (100.0, 400.0, np.array([7.5, 7.5])),
    12: (290.0, 12.5, np.array([30.0, 22.0, 41.0, 18.0, 18.0, 25.0, 60.0])),
}
HEAT_REFS = (100.0, 450.25, 600.0)                     # T_ref of the stored heat: below every table, inside some, above some
CV_ORDER = [8, 3, 11, 5, 7]
K_ORDER = [12, 3, 11, 7]
TAG_K = {2: 40.0, 3: 9.0, 5: 3.5, 7: 15.0, 8: 1.2, 11: 80.0, 12: 25.0}
TAG_RC = {2: 1.7e6, 3: 2.1e6, 5: 2.6e6, 7: 1.9e6, 8: 2.3e6, 11: 3.3e6, 12: 1.4e6}
TAGS = sorted(TAG_K)                                   # the tag dictionary: ascending

NZN, NRN, H = 127, 80, 2.0e-8                          # nodes along z and r, spacing
PER_ROW = NRN // 4                                     # patches per block row
BLOCK_ROWS = {2: 0, 3: 4, 5: 4, 7: 6, 8: 6, 11: 6, 12: 2}


def ulps(x, m):
    """x moved by m float64 steps."""
    x = np.float64(x)
    for _ in range(abs(int(m))):
        x = np.nextafter(x, np.inf if m > 0 else -np.inf)
    return float(x)


def knot_float(tab, k):
    """The float64 nearest to knot k of an ExactTable."""
    return float(tab.knot(k))


def special_knots(n):
    return sorted({0, 1, n // 2, n - 2, n - 1} & set(range(n)))


def designed_points(tab):
    """Arguments of the plain table value: every special knot and 1 and 8 ulp to either side, and one in each region."""
    T0, dT, n = tab.T0, tab.dT, tab.n
    out = [ulps(knot_float(tab, k), m) for k in special_knots(n) for m in (-8, -1, 0, 1, 8)]
    return out + [T0 - 0.6 * dT - 2.0, T0 + 0.37 * dT, T0 + (n - 1) * dT + 0.6 * dT + 2.0]


def designed_pairs(tab):
    """The pair list of one table; every other pair is handed over as (hi, lo)."""
    T0, dT, n = tab.T0, tab.dT, tab.n
    Tend = T0 + (n - 1) * dT
    out = [(T, T) for T in designed_points(tab)]
    for k in special_knots(n):
        Tk = knot_float(tab, k)
        for d in (None, 1e-9 * dT, 0.3 * dT):
            lo, hi = (ulps(Tk, -1), ulps(Tk, 1)) if d is None else (Tk - d, Tk + d)
            out += [(lo, hi), (Tk, hi), (lo, Tk)]
    if n >= 4:
        out += [(T0 + 0.4 * dT, T0 + 2.6 * dT), (Tend - 2.7 * dT, Tend - 0.2 * dT), (T0 + (n // 2 - 1.5) * dT, T0 + (n // 2 + 1.25) * dT)]
    out += [(T0 - 3.0 * dT - 5.0, T0 - 0.5 * dT - 1.0), (Tend + 0.5 * dT + 1.0, Tend + 3.0 * dT + 5.0),
            (T0 - 0.7 * dT, T0 + 0.4 * dT), (Tend - 0.4 * dT, Tend + 0.7 * dT), (T0 - 0.1 * (Tend - T0) - 1.0, Tend + 0.1 * (Tend - T0) + 1.0),
            (T0 - 0.7 * dT, T0 + 0.5 * (Tend - T0) + 0.21 * dT), (T0 + 0.5 * (Tend - T0) - 0.21 * dT, Tend + 0.7 * dT)]
    out += knot_end_pairs(tab)
    return [(b, a) if q % 2 else (a, b) for q, (a, b) in enumerate(out)]


KNOT_END_PATCHES = 3          # patches per knot-end class: Tw_e keeps a patch's value to the last bit in about a third of its triangles


def knot_end_pairs(tab):
    """Pairs with one end exactly on a knot that is a float64 and the other end in a later or earlier piece: from below the table
    onto an inner knot, from a knot to above the table, and from a knot over one and over two knots (and their mirrors).  With sl
    on a knot ktab_mean's head piece is a whole first segment (x = 0), with sh on one its tail piece is empty.  Each class
    KNOT_END_PATCHES times, over the float64 knots in turn."""
    T0, dT, n = tab.T0, tab.dT, tab.n
    Tend = T0 + (n - 1) * dT
    fk = tab.float_knots()
    K = {k: float(tab.knot(k)) for k in fk}

    def turns(ks):
        ks = list(ks)
        return [ks[(q * max(1, len(ks) // KNOT_END_PATCHES)) % len(ks)] for q in range(KNOT_END_PATCHES)] if ks else []
    out = [(T0 - 0.7 * dT, K[k]) for k in turns(k for k in fk if k >= 1)]                         # below_into_interior+knot
    out += [(K[k], Tend + 0.7 * dT) for k in turns(k for k in fk if k <= n - 2)]                  # interior_into_above+knot
    for reach, need in ((1.4, 3), (2.6, 4)):                                                       # straddle_one_knot+knot, span_knots+knot
        if n >= need:
            up, down = [k for k in fk if k + reach <= n - 1], [k for k in fk if k - reach >= 0]
            both = [(K[k], K[k] + reach * dT) for k in up] + [(K[k] - reach * dT, K[k]) for k in down]
            out += turns(both[::2] + both[1::2])
    return out


def exact_tables(tables):
    return {t: ExactTable(*v) for t, v in tables.items()}


def patch_list(tag):
    """The (Ta, Tb) of the band's patches: the capacity table's pairs, for every reference temperature of the stored heat inside
    the table three values beside it (the same segment, one knot on, two knots on), then the conductivity table's points, as (T, T)."""
    out = []
    if tag in CV_TABLES:
        tab = ExactTable(*CV_TABLES[tag])
        out += designed_pairs(tab)
        out += [(T + d * tab.dT, T + d * tab.dT) for T in HEAT_REFS if tab.classify_point(T) == "segment" for d in (1e-3, 1.0, 2.5)]
    if tag in K_TABLES:
        out += [(T, T) for T in designed_points(ExactTable(*K_TABLES[tag]))]
    return out


def _bands():
    """{tag: (first node row, rows)}: a margin row, the block rows, one row of random fill (and the patches no pair takes)."""
    out, row = {}, 0
    for t in TAGS:
        rows = 1 + 4 * BLOCK_ROWS[t] + 1
        out[t] = (row, rows)
        row += rows
    assert row <= NZN - 1, row
    return out


def build_mesh(seed=5):
    """(coords, tris, tags, bc_dofs)."""
    rng = np.random.default_rng(seed)
    Z, R = np.meshgrid(H * np.arange(NZN), H * np.arange(NRN), indexing="ij")
    coords = np.column_stack([Z.ravel(), R.ravel()])
    inner = (Z.ravel() > 0) & (Z.ravel() < H * (NZN - 1)) & (R.ravel() > 0) & (R.ravel() < H * (NRN - 1))
    coords[inner] += rng.uniform(-0.3, 0.3, (int(inner.sum()), 2)) * H
    idx = lambda i, j: i * NRN + j
    cells = [(i, j) for i in range(NZN - 1) for j in range(NRN - 1)]
    tris = np.array([[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)] for i, j in cells] +
                    [[idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)] for i, j in cells], dtype=np.int32)
    row_of = np.array([i for i, _ in cells] * 2)
    tags = np.full(len(tris), TAGS[-1], dtype=np.int32)
    for t, (r0, rows) in _bands().items():
        tags[(row_of >= r0) & (row_of < r0 + rows)] = t
    flip = rng.random(len(tris)) < 0.5
    tris[flip] = tris[flip][:, [0, 2, 1]]
    perm = rng.permutation(len(tris))
    bc = np.sort(rng.choice(len(coords), size=23, replace=False)).astype(np.int32)
    return coords, tris[perm], tags[perm], bc


def _fill_range(tag):
    spans = [(v[0], v[0] + (len(v[2]) - 1) * v[1]) for tab in (CV_TABLES, K_TABLES) if tag in tab for v in [tab[tag]]]
    if not spans:
        return 250.0, 900.0
    lo, hi = min(s[0] for s in spans), max(s[1] for s in spans)
    return lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo)


def build_states(seed=9, rotate=0):
    """(u^n, e) of NZN * NRN values each."""
    rng = np.random.default_rng(seed)
    un, e = np.empty((NZN, NRN)), np.empty((NZN, NRN))
    for t, (r0, rows) in _bands().items():
        lo, hi = _fill_range(t)
        un[r0:r0 + rows + 1] = rng.uniform(lo, hi, (rows + 1, NRN))
        e[r0:r0 + rows + 1] = rng.uniform(lo, hi, (rows + 1, NRN))
    last = _bands()[TAGS[-1]]
    lo, hi = _fill_range(TAGS[-1])
    un[last[0] + last[1]:] = rng.uniform(lo, hi, un[last[0] + last[1]:].shape)
    e[last[0] + last[1]:] = rng.uniform(lo, hi, e[last[0] + last[1]:].shape)
    for t, (r0, rows) in _bands().items():
        pairs = patch_list(t)
        slots = BLOCK_ROWS[t] * PER_ROW
        assert len(pairs) <= slots, (t, len(pairs), slots)
        for q, (Ta, Tb) in enumerate(pairs):
            a, b = divmod((q + rotate * 7) % slots, PER_ROW)
            i0, j0 = r0 + 1 + 4 * a, 4 * b
            un[i0:i0 + 4, j0:j0 + 4] = Ta
            e[i0:i0 + 4, j0:j0 + 4] = Tb
    return un.ravel().copy(), e.ravel().copy()


def class_counts(tab, Ta, Tb=None):
    """{class: triangles} of the exact classifier over arrays of element temperatures (points where Tb is None)."""
    out = {}
    if Tb is None:
        for T in Ta:
            c = tab.classify_point(T)
            out[c] = out.get(c, 0) + 1
        return out
    for a, b in zip(Ta, Tb):
        c = tab.classify_pair(a, b)
        out[c] = out.get(c, 0) + 1
        if c.endswith("+knot"):                                            # an end on a knot also counts for its base class
            out[c[:-5]] = out.get(c[:-5], 0) + 1
    return out


MIN_TRIANGLES = 8


def missing_classes(counts, wanted):
    return {c: counts.get(c, 0) for c in wanted if counts.get(c, 0) < MIN_TRIANGLES}
