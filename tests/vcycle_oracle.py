"""Float64 restatements of the multigrid preconditioner B (one V(1,1) cycle, heatflow_amd/csrc/hf_solver.hpp vcycle()).

* stored_cycle: the cycle the way the code launches it, with the operators a hierarchy blob stores (tests/amg_blob.py),
  promoted to f64 without rounding, and every vector operation in f64.  The device differs from it only in the order of
  its sums (its kernels multiply double(val) * x and accumulate in double), so it is a tight reference.
* definition_cycle: the textbook V(1,1) cycle built from its parts A_l, P_l, R_l := P_l^T, D_l, w_l, with a direct solve
  on the coarsest level and the fused legs replaced by their definitions
      Rt_l = R_l (I - w A_l D_l^-1),   GP_l = [2 w D^-1 - w^2 D^-1 A D^-1 | (I - w D^-1 A) P].
  It catches a fused leg or a coarse inverse that is self-consistent but belongs to another operator.
* galerkin_errors: the algebra the blob must satisfy (A_{l+1} = R_l A_l P_l, R_l = P_l^T, the coarse inverse).

Levels are dicts {"n", "omega", "dinv", "A", "P", "R", "Rt", "GP"} whose operators are scipy matrices (or None); the
blob's Operator objects are accepted as well.  Level 0's A and D^-1 are the context's own (hf_get_csr), not in the blob."""
import numpy as np
import scipy.linalg
import scipy.sparse as sp


def _m(op):
    if op is None:
        return None
    return op.M if hasattr(op, "M") else op


def fine_operator(be):
    """(A, D^-1) of the context's assembled fine operator, as the device holds them (D^-1 = 1 / diag, k_dinv)."""
    rowptr, colidx, A, _ = be.get_csr()
    S = sp.csr_matrix((A, colidx, rowptr), shape=(be.n, be.n))
    return S, 1.0 / S.diagonal()


def coarse_apply(H, b):
    """The coarsest level as vcycle() runs it: the stored dense inverse (rounded to f32 when the hierarchy is f32) or,
    without one, w D^-1 b."""
    Lc = H["levels"][-1]
    if H["coarse_inv"] is None:
        return Lc["omega"] * Lc["dinv"] * b
    n = H["header"]["coarse_n"]
    X = H["coarse_inv"][:, :n]
    if H["header"]["f32"]:
        X = X.astype(np.float32).astype(np.float64)
    return X @ b


def stored_cycle(H, A0, dinv0, r, stale=False, explicit=False, post=True):
    """z = B r with the blob's stored operators.  ``stale``: the fine operator was re-valued under the frozen hierarchy
    (hf_update_kappa with reuse): a fused down leg alone gives way to the explicit one over the new A0 (vcycle()).
    ``explicit``: both finest legs explicit whatever the blob holds (the batched cycle, BatchOps::vcycle).  ``post`` = False (with
    ``explicit``): the finest level's post-smoothing sweep is left out - a non-symmetric B, the fault tests/pcg_oracle.py injects."""
    L = H["levels"]
    nl = len(L)
    w0 = L[0]["omega"]
    z0 = w0 * (dinv0 * r)                              # what k_pcg_update_amg leaves: w * (D^-1 r)
    assert post or explicit
    if nl == 1:
        return z0 + w0 * dinv0 * (r - A0 @ z0) if post else z0
    fused0 = L[0]["GP"] is not None and not explicit
    b = [None] * nl
    if L[0]["Rt"] is not None and not explicit and (fused0 or not stale):
        b[1] = _m(L[0]["Rt"]) @ r
    else:
        b[1] = _m(L[0]["R"]) @ (r - A0 @ z0)
    for l in range(1, nl - 1):
        b[l + 1] = _m(L[l]["Rt"]) @ b[l]
    x = coarse_apply(H, b[nl - 1])
    for l in range(nl - 2, 0, -1):
        x = _m(L[l]["GP"]) @ np.concatenate([b[l], x])
    if fused0:
        return _m(L[0]["GP"]) @ np.concatenate([r, x])
    z = z0 + _m(L[0]["P"]) @ x
    return z + w0 * dinv0 * (r - A0 @ z) if post else z


def definition_cycle(H, A0, dinv0, r, coarse_solve=None):
    """z = B r of the textbook V(1,1) cycle on the levels' A, P, P^T, D^-1, w (the blob's values; level 0 from A0 /
    dinv0 and the blob's w_0); coarsest level by a direct solve on A_c (or w D^-1 b when the hierarchy has no inverse)."""
    L = H["levels"]
    nl = len(L)
    if coarse_solve is None and H["coarse_inv"] is not None and nl > 1:
        Ac = _m(L[-1]["A"]).toarray()
        coarse_solve = lambda b: scipy.linalg.solve(Ac, b, assume_a="pos")  # noqa: E731

    def level(l, b):
        A = A0 if l == 0 else _m(L[l]["A"])
        d = dinv0 if l == 0 else L[l]["dinv"]
        w = L[l]["omega"]
        if l == nl - 1 and l > 0:
            return coarse_solve(b) if coarse_solve is not None else w * d * b
        x = w * d * b
        if l < nl - 1:
            P = _m(L[l]["P"])
            x = x + P @ level(l + 1, P.T @ (b - A @ x))
        return x + w * d * (b - A @ x)

    return level(0, r)


def fused_leg_definitions(H, A0, dinv0):
    """{(level, "Rt" / "GP"): (stored, definition)} for every fused leg of the blob (level 0 against A0 / dinv0)."""
    out = {}
    for l, Lv in enumerate(H["levels"][:-1]):
        A = A0 if l == 0 else _m(Lv["A"])
        d = dinv0 if l == 0 else Lv["dinv"]
        w = Lv["omega"]
        P = _m(Lv["P"])
        D = sp.diags(d)
        Pt = P - w * (D @ (A @ P))
        if Lv["Rt"] is not None:
            out[(l, "Rt")] = (_m(Lv["Rt"]), Pt.T.tocsr())
        if Lv["GP"] is not None:
            G = 2 * w * D - w * w * (D @ A @ D)
            out[(l, "GP")] = (_m(Lv["GP"]), sp.hstack([G, Pt]).tocsr())
    return out


def _row_rel(E, S):
    """max over rows of max|E_row| / max|S_row|."""
    E, S = abs(sp.csr_matrix(E)), abs(sp.csr_matrix(S))
    em = E.max(axis=1).toarray().ravel()
    sm = S.max(axis=1).toarray().ravel()
    sm[sm == 0] = 1.0
    return float((em / sm).max()) if em.size else 0.0


def galerkin_errors(H, A0):
    """Measured algebra of the blob: {"galerkin": [per level l: max over rows of |R A P - A_{l+1}| / max|A_{l+1} row|],
    "transpose": [per level: max |R - P^T|], "coarse_backward": ||A_c X - I||_max / (||A_c|| ||X||) (inf-norms),
    "coarse_symmetry": max|X - X^T| / max|X|}."""
    L = H["levels"]
    out = {"galerkin": [], "transpose": []}
    for l in range(len(L) - 1):
        A = A0 if l == 0 else _m(L[l]["A"])
        P, R = _m(L[l]["P"]), _m(L[l]["R"])
        Ac = _m(L[l + 1]["A"])
        out["galerkin"].append(_row_rel(R @ A @ P - Ac, Ac))
        out["transpose"].append(float(abs(R - P.T.tocsr()).max()) if R.nnz else 0.0)
    if H["coarse_inv"] is not None:
        n = H["header"]["coarse_n"]
        X = H["coarse_inv"][:, :n]
        Ac = _m(L[-1]["A"]).toarray()
        E = Ac @ X - np.eye(n)
        out["coarse_backward"] = float(np.abs(E).max() / (np.abs(Ac).sum(1).max() * np.abs(X).sum(1).max()))
        out["coarse_symmetry"] = float(np.abs(X - X.T).max() / np.abs(X).max())
        out["coarse_pad"] = float(np.abs(H["coarse_inv"][:, n:]).max()) if H["header"]["coarse_ld"] > n else 0.0
    return out


def rel_max(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def check_context(be, vectors, stale=False, fine_def=None):
    """Apply the device cycle of context ``be`` (hf_amg_apply) to each named vector and measure it against both
    restatements of the hierarchy the context exports.  ``fine_def``: (A, D^-1) of the definition's finest level when it
    is not the context's current operator (frozen hierarchy with both legs fused: the cycle of the OLD operator).
    Returns the hierarchy and {"stored": worst relative error against stored_cycle, "definition": against
    definition_cycle, "rz": worst |rz - r.z| / sum|r_i z_i|, "rz_stored": worst |rz - r.z_ref| / |r.z_ref|,
    "bitwise": both applications identical, "finite": no NaN / Inf, "per_vector": {...}}."""
    H = parse_export(be)
    A0, d0 = fine_operator(be)
    Ad, dd = fine_def if fine_def is not None else (A0, d0)
    out = {"stored": 0.0, "definition": 0.0, "rz": 0.0, "rz_stored": 0.0, "bitwise": True, "finite": True, "per_vector": {}}
    for name, r in vectors.items():
        z, rz = be.amg_apply(r)
        z2, rz2 = be.amg_apply(r)
        out["bitwise"] &= bool(np.array_equal(z, z2) and rz == rz2)
        out["finite"] &= bool(np.isfinite(z).all() and np.isfinite(rz))
        zs = stored_cycle(H, A0, d0, r, stale=stale)
        zd = definition_cycle(H, Ad, dd, r)
        e = {"stored": rel_max(z, zs), "definition": rel_max(z, zd),
             "rz": abs(rz - float(r @ z)) / float(np.abs(r * z).sum()), "rz_stored": abs(rz - float(r @ zs)) / abs(float(r @ zs))}
        out["per_vector"][name] = e
        for k in ("stored", "definition", "rz", "rz_stored"):
            out[k] = max(out[k], e[k])
    return H, out


def symmetry_and_positivity(apply, n, seed=5):
    """(max |x.By - y.Bx| / sqrt(x.Bx y.By) over two pairs, min x.Bx / |x|^2 over five random vectors)."""
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal(n) for _ in range(5)]
    zs = [apply(x) for x in xs]
    q = [float(x @ z) for x, z in zip(xs, zs)]
    sym = 0.0
    for i, j in ((0, 1), (2, 3)):
        sym = max(sym, abs(float(xs[i] @ zs[j]) - float(xs[j] @ zs[i])) / np.sqrt(abs(q[i] * q[j])))
    return sym, min(qi / float(x @ x) for qi, x in zip(q, xs))


def parse_export(be):
    import amg_blob

    return amg_blob.parse(be.amg_export())


def kernel_table(text):
    """The set-up's operator table under HEATFLOW_DEBUG ("[amg] level 1 GP ... stream rpc 64 lanes 32 f32 c16"):
    [(level, operator, "stream" / "vec", rpc, lanes, "f32" / "f64", c16)]."""
    import re

    return [(int(m[0]), m[1], m[2], int(m[3]), int(m[4]), m[5], bool(m[6]))
            for m in re.findall(r"\[amg\] level (\d+) (\w+) .*? (stream|vec) rpc (\d+) lanes (\d+) (f32|f64)( c16)?", text)]


def operator_table(H):
    """[(level, operator, "stream" / "vec", rpc, lanes, "f32" / "f64", c16)] of the blob's records - the kernel each
    operator runs through (rpc > 0: the LDS-staged k_spmv, else k_spmv_vec at `lanes`), as the HEATFLOW_DEBUG table."""
    out = []
    for l, L in enumerate(H["levels"]):
        for name in ("A", "P", "R", "Rt", "GP"):
            op = L[name]
            if op is not None:
                r = op.record
                out.append((l, name, "stream" if r["rpc"] else "vec", r["rpc"], r["lanes"], "f32" if op.f32 else "f64",
                            bool(r["has_c16"])))
    return out


def differing_operators(Ha, Hb):
    """["level l OP", ..., "coarse inverse"]: the stored operators whose values differ between two hierarchies."""
    out = []
    for l, (La, Lb) in enumerate(zip(Ha["levels"], Hb["levels"])):
        for name in ("A", "P", "R", "Rt", "GP"):
            a, b = _m(La[name]), _m(Lb[name])
            if (a is None) != (b is None) or (a is not None and (a.shape != b.shape or abs(a - b).max() != 0)):
                out.append(f"level {l} {name}")
    if (Ha["coarse_inv"] is None) != (Hb["coarse_inv"] is None) or (
            Ha["coarse_inv"] is not None and not np.array_equal(Ha["coarse_inv"], Hb["coarse_inv"])):
        out.append("coarse inverse")
    return out


def test_vectors(prob, seed=1):
    """{"random": unit normal, "smooth": a smooth field over the mesh, "step": the residual b - A u^n of the start of the
    next step after two real ones (the start vector u^n, the right-hand side M u^n on the free rows)}."""
    n = prob.n
    rng = np.random.default_rng(seed)
    z, rr = prob.coords[:, 0], prob.coords[:, 1]
    zs = (z - z.min()) / max(np.ptp(z), 1e-300)
    rs = (rr - rr.min()) / max(np.ptp(rr), 1e-300)
    for bc in prob.bcs:
        bc.update(0.0)
    for k in range(2):
        prob.step((k + 1) * prob.dt, only=[prob.bcs[3]])
    rowptr, colidx, A, M = prob.backend.get_csr()
    u = prob.state()
    Am = sp.csr_matrix((A, colidx, rowptr), shape=(n, n))
    Mm = sp.csr_matrix((M, colidx, rowptr), shape=(n, n))
    step = Mm @ u - Am @ u
    step[prob.bc_dofs] = 0.0
    if not np.abs(step).max() > 0:
        step = rng.standard_normal(n)
    return {"random": rng.standard_normal(n), "smooth": np.sin(3.0 * zs) * np.cos(2.0 * rs) + zs * rs,
            "step": step / np.abs(step).max()}


def run_case(spec):
    """One hierarchy case end to end (used in the test process and in child processes for the settings the library reads
    once).  spec: {"case", "scale", "reuse": bool, "kappa": factor on the sample's conductivity after the set-up (frozen
    hierarchy), "scheme"}.  Returns a JSON-able dict: header, operator table, check_context metrics, algebra,
    symmetry / positivity."""
    import os
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    from conftest import build_case
    from helpers import make_problem, material_tables

    cfg, stack, mesh = build_case(spec["case"], spec["scale"])
    prob = make_problem(cfg, stack, mesh, precond=1, amg_reuse=bool(spec.get("reuse")),
                        scheme=spec.get("scheme", "backward_euler"))
    try:
        be = prob.backend
        vecs = test_vectors(prob)
        stale, fine_def = False, None
        H0 = parse_export(be)
        A_built, d_built = fine_operator(be)
        if spec.get("kappa"):
            tag_to_k, _ = material_tables(stack, mesh)
            tag = mesh.material_tags["p_sample"] if "p_sample" in mesh.material_tags else sorted(tag_to_k)[0]
            be.update_kappa([tag], [tag_to_k[tag] * float(spec["kappa"])])
            stale = True
            if H0["levels"][0]["GP"] is not None:       # both legs fused: the cycle of the old operator
                fine_def = (A_built, d_built)
        H, m = check_context(be, vecs, stale=stale, fine_def=fine_def)
        assert differing_operators(H, H0) == [], "the frozen hierarchy changed"
        alg = galerkin_errors(H, A_built)
        sym, pos = symmetry_and_positivity(lambda x: be.amg_apply(x)[0], be.n)
        installed = None
        if spec.get("install"):                      # the exported blob installs on a fresh context: the same cycle, bit for bit
            other = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True, amg=be.amg_export())
            try:
                installed = all(np.array_equal(other.backend.amg_apply(r)[0], be.amg_apply(r)[0]) for r in vecs.values())
            finally:
                other.close()
        h = H["header"]
        return {"installed": installed, "pipeline": stream_pipeline(H), "n": be.n, "nl": h["nl"], "fuse0": h["fuse0"], "f32": h["f32"], "coarse_n": h["coarse_n"],
                "rows": [L["n"] for L in H["levels"]], "table": operator_table(H), "metrics": m, "algebra": alg,
                "symmetry": sym, "positivity": pos, "stale": stale, "old_operator": fine_def is not None}
    finally:
        prob.close()


TS = 512   # rows per chunk at most and threads of the LDS-staged kernel (hf_context.hpp)


def stream_pipeline(H):
    """[(level, operator, UN, second_pass)] for every operator the LDS-staged kernel runs through its chunk pipeline
    (f32 values with a compressed column stream): UN = 4 stream entries per lane in flight where the average chunk
    holds at most 3.5 per lane (short_chunks(), hf_solver.hpp), else 8; second_pass = a chunk longer than UN * TS
    entries, whose remainder the kernel takes in a second, unpipelined loop."""
    out = []
    for l, L in enumerate(H["levels"]):
        for name in ("A", "P", "R", "Rt", "GP"):
            op = L[name]
            if op is None or not op.record["rpc"] or not op.f32 or op.c16 is None:
                continue
            r = op.record
            un = 4 if r["nnz"] <= r["nchunks"] * (7 * TS // 2) else 8
            out.append((l, name, un, bool(r["chunk_nnz"] > un * TS)))
    return out


def batch_columns_per_lane(nv, op):
    """Columns per lane the batched CSR launch gives operator ``op`` (blaunch_csr, hf_batch.hpp): nv -> kb_csr, fewer
    -> kb_csr_rc (default settings)."""
    nrow, nnz = op.record["nrow"], op.record["nnz"]
    avg = nnz / nrow if nrow else 1.0
    return 4 if nv >= 8 and nrow >= 1024 and not (nv == 8 and nrow < 4096 and avg < 64.0) else nv


def locate(z_gpu, H_ref, H_bad, A0, dinv0, r, tol):
    """Which stored operator explains a device cycle that misses the restatement of ``H_ref``: for every operator of the
    hierarchy (and the coarse inverse), the stored restatement with that one operator taken from ``H_bad``; returns
    ["level l OP" / "coarse inverse" whose swap brings the restatement within ``tol`` of z_gpu]."""
    import copy

    named = []
    for l, L in enumerate(H_ref["levels"]):
        for name in ("P", "R", "Rt", "GP") + (("A",) if l > 0 else ()):
            if L[name] is None:
                continue
            H = copy.copy(H_ref)
            H["levels"] = [dict(Lv) for Lv in H_ref["levels"]]
            H["levels"][l][name] = H_bad["levels"][l][name]
            if rel_max(z_gpu, stored_cycle(H, A0, dinv0, r)) <= tol:
                named.append(f"level {l} {name}")
    if H_ref["coarse_inv"] is not None:
        H = dict(H_ref, coarse_inv=H_bad["coarse_inv"])
        if rel_max(z_gpu, stored_cycle(H, A0, dinv0, r)) <= tol:
            named.append("coarse inverse")
    return named
