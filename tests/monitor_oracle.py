"""Float64 restatement of the region monitors (hf_set_monitors).  TEST CODE.

Per triangle the three terms are formed with the operations of k_monitor in their pinned order (numpy evaluates one IEEE
operation per ufunc call, nothing is contracted); per tag they are summed with math.fsum, so only the order of summation
differs from the device.  The extremes are exact: the largest / smallest nodal value over the nodes of the tag's triangles and
the smallest node id that attains it.
"""
import math

import numpy as np

FIELDS = ("T_max", "node_max", "T_min", "node_min", "I0", "I1", "H")
EPS = 2.0 ** -52


def triangle_terms(coords, tris, u, theta):
    """(I0_e, I1_e, H_e, nodes above) of every triangle; ``theta`` per triangle (+inf: nothing is above)."""
    coords = np.asarray(coords, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64)
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64), (len(tris),))
    z = coords[tris, 0]
    r = coords[tris, 1]
    uu = u[tris]
    z0, z1, z2 = z[:, 0], z[:, 1], z[:, 2]
    r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
    u0, u1, u2 = uu[:, 0], uu[:, 1], uu[:, 2]
    d = (z1 - z0) * (r2 - r0) - (z2 - z0) * (r1 - r0)
    A = 0.5 * np.abs(d)
    rs = (r0 + r1) + r2
    I0 = (A * rs) / 3.0
    I1 = (A / 12.0) * (((rs + r0) * u0 + (rs + r1) * u1) + (rs + r2) * u2)
    above = uu > theta[:, None]
    cnt = above.sum(axis=1)
    odd = cnt == 1                                   # the odd node out is the one above; with two above, the one not above
    a = np.where(above[:, 0] == odd, 0, np.where(above[:, 1] == odd, 1, 2))
    rows = np.arange(len(tris))
    b, c = (a + 1) % 3, (a + 2) % 3
    ua, ub, uc = uu[rows, a], uu[rows, b], uu[rows, c]
    ra, rb, rc = r[rows, a], r[rows, b], r[rows, c]
    cut_case = (cnt == 1) | (cnt == 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        sb = (ua - theta) / (ua - ub)
        sc = (ua - theta) / (ua - uc)
        cut = (((A * sb) * sc) * ((ra + (ra + sb * (rb - ra))) + (ra + sc * (rc - ra)))) / 3.0
        H = np.where(cnt == 0, 0.0, np.where(cnt == 3, I0, np.where(odd, cut, I0 - cut)))
    H = np.where(cut_case | (cnt == 3), H, 0.0)
    return I0, I1, H, cnt


def per_tag(coords, tris, tags, u, thresholds, tab_len=None):
    """The record [tab_len, 7] of HeatflowHIP.monitor_now for ``thresholds`` = {cell tag: theta | None (+inf)}, and per tag:
    ``scale`` [tab_len, 3] = sum_e |term_e| of I0, I1 and H, ``ne`` [tab_len] = triangles of the tag, ``branches`` [tab_len, 4] =
    triangles with 0, 1, 2, 3 nodes above the tag's threshold."""
    tags = np.asarray(tags, dtype=np.int64)
    tris = np.asarray(tris, dtype=np.int64)
    u = np.asarray(u, dtype=np.float64)
    tab_len = int(tags.max()) + 1 if tab_len is None else int(tab_len)
    th_tag = np.full(tab_len, np.nan)
    for t, th in thresholds.items():
        th_tag[int(t)] = math.inf if th is None else float(th)
    monitored = ~np.isnan(th_tag[tags])
    theta = np.where(monitored, th_tag[tags], math.inf)
    I0, I1, H, cnt = triangle_terms(coords, tris, u, theta)
    rec = np.zeros((tab_len, 7))
    scale = np.zeros((tab_len, 3))
    ne = np.zeros(tab_len, dtype=np.int64)
    branches = np.zeros((tab_len, 4), dtype=np.int64)
    for t in sorted(int(t) for t in thresholds):
        sel = tags == t
        if not sel.any():
            raise ValueError(f"tag {t} is not a cell tag of the mesh")
        nodes = np.unique(tris[sel])
        vals = u[nodes]
        rec[t, 0] = vals.max()
        rec[t, 1] = nodes[vals == vals.max()].min()
        rec[t, 2] = vals.min()
        rec[t, 3] = nodes[vals == vals.min()].min()
        for f, term in enumerate((I0, I1, H)):
            rec[t, 4 + f] = math.fsum(term[sel])
            scale[t, f] = math.fsum(np.abs(term[sel]))
        ne[t] = int(sel.sum())
        branches[t] = np.bincount(cnt[sel], minlength=4)
    return rec, scale, ne, branches


def sum_bound(ne, scale):
    """(ne_t + 16) 2^-52 sum_e |term_e|: any order of summation of ne_t terms costs at most (ne_t - 1) eps sum |term|, and a term
    carries a few roundings of its own."""
    return (np.asarray(ne, dtype=np.float64)[..., None] + 16.0) * EPS * np.asarray(scale)


def energy(rec, rho_c, T_ref):
    """2 pi sum_t rho_c_t (I1_t - T_ref I0_t) over the tags of ``rho_c``, ascending."""
    e = 0.0
    for t in sorted(rho_c):
        e = e + float(rho_c[t]) * (rec[t, 5] - float(T_ref) * rec[t, 4])
    return 2.0 * math.pi * e
