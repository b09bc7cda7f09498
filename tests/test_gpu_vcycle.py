"""The multigrid preconditioner B (one V(1,1) cycle) as the device applies it, against float64 restatements of the same
operator (tests/vcycle_oracle.py) on the hierarchy the context exports (tests/amg_blob.py).

PCG converges to the same answer with any SPD preconditioner, so field-versus-oracle tests cannot see a wrong B; these
compare z = B r itself (hf_amg_apply, hf_batch_apply_precond) and the coarsest level's dense inverse (hf_dense_inverse).

Tolerances (worst values measured on an MI355X are recorded in each test's docstring):
  STORED      max|z_gpu - z_stored| <= 1e-11 max|z_stored|: the device and the stored-operator restatement differ only in
              summation order; one wrong f32 entry moves z by 1e-7 or more.
  RZ          the r.z sum the cycle leaves for PCG against r.z_gpu, relative to sum|r_i z_i|: 1e-12.
  DEF_F32     against the textbook cycle (definition restatement) with f32 transfer operators: 1e-5; DEF_F64 with f64: 1e-9.
  SYM         |x.By - y.Bx| / sqrt(x.Bx y.By): 1e-6 (f32 operators), and x.Bx > 0 on five random vectors.
Settings the library reads once per process (HEATFLOW_STREAM_MIN_ROWS, HEATFLOW_STREAM_NNZ, HEATFLOW_BATCH_DENSE_CPL)
run in child processes, one at a time, each under a time limit; the others use monkeypatch.

k_spmv_row (a workgroup per row) needs an average of more than 128 entries per row with default lane scaling: no
operator of these hierarchies reaches it, and no knob short of HEATFLOW_VEC_PER_LANE (which changes the scaling itself,
never selecting lanes > 64) does; it is left unreached here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
import amg_blob
import vcycle_oracle as vo

pytestmark = pytest.mark.gpu

STORED, RZ, DEF_F32, DEF_F64, SYM = 1e-11, 1e-12, 1e-5, 1e-9, 1e-6
KNOBS = ("HEATFLOW_AMG_FUSE0", "HEATFLOW_AMG_F32", "HEATFLOW_AMG_COARSE", "HEATFLOW_SPMV_C16", "HEATFLOW_STREAM_MIN_ROWS",
         "HEATFLOW_STREAM_NNZ", "HEATFLOW_BATCH_DENSE_CPL", "HEATFLOW_VEC_PER_LANE")


@pytest.fixture
def clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def check(res, what):
    """The assertions every case makes on a run_case result; prints the measured values."""
    m, alg = res["metrics"], res["algebra"]
    f32 = bool(res["f32"])
    assert m["finite"], f"{what}: NaN in z (an entry of a level vector read before it is written)"
    assert m["bitwise"], f"{what}: two applications of B differ"
    assert m["stored"] <= STORED, (what, "stored-operator restatement", m["per_vector"])
    assert m["rz"] <= RZ and m["rz_stored"] <= 1e-10, (what, "r.z partial slots", m["per_vector"])
    assert m["definition"] <= (DEF_F32 if f32 else DEF_F64), (what, "definition restatement", m["per_vector"])
    assert res["symmetry"] <= (SYM if f32 else 1e-9) and res["positivity"] > 0.0, (what, res["symmetry"], res["positivity"])
    for l, e in enumerate(alg["galerkin"]):
        assert e <= (1e-5 if f32 else 1e-12), (what, f"A_{l + 1} = R_{l} A_{l} P_{l}", alg["galerkin"])
    assert all(t == 0.0 for t in alg["transpose"]), (what, "R = P^T", alg["transpose"])
    if res["coarse_n"] > 0:
        assert alg["coarse_backward"] <= 1e-10 and alg["coarse_symmetry"] <= 1e-12 and alg["coarse_pad"] == 0.0, (what, alg)
    print(f"{what}: n={res['n']} rows={res['rows']} fuse0={res['fuse0']} f32={res['f32']} stored={m['stored']:.2e} "
          f"def={m['definition']:.2e} rz={m['rz']:.2e} sym={res['symmetry']:.2e} galerkin={max(alg['galerkin'] or [0]):.2e} "
          f"coarse={alg.get('coarse_backward', 0):.2e}")


def child(spec, env, tmp_path, name, timeout=900):
    """run_case in a fresh process with ``env`` (settings read once per process) and HEATFLOW_DEBUG=1; returns its result
    and the kernel table the set-up printed."""
    script = tmp_path / f"{name}.py"
    out = tmp_path / f"{name}.json"
    script.write_text(
        "import json, sys\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "import vcycle_oracle\n"
        f"res = vcycle_oracle.run_case({spec!r})\n"
        f"open({str(out)!r}, 'w').write(json.dumps(res))\n")
    full = {k: v for k, v in os.environ.items() if k not in KNOBS}
    full.update(env, HEATFLOW_DEBUG="1")
    res = subprocess.run([sys.executable, str(script)], env=full, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, (name, res.returncode, res.stderr[-3000:])
    data = json.loads(out.read_text())
    printed = vo.kernel_table(res.stdout + res.stderr)
    assert sorted(map(tuple, printed)) == sorted(map(tuple, data["table"])), (name, "HEATFLOW_DEBUG table against the blob")
    return data


def streamed(res, level, op):
    return [t for t in res["table"] if t[0] == level and t[1] == op and t[2] == "stream"]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["geballe_with_diamond", "geballe_no_diamond"])
def test_stock_small_mesh_cycle(hip, clean_env, case):
    """Default settings at mesh scale 8: every operator through the sub-wave kernels (k_spmv_vec), the finest level
    explicit (its fused legs are dropped below the stream kernel's size), k_dense_mv_f32 on the coarsest level.
    Measured (2 levels): stored 5.3e-16, definition 2.0e-8, r.z 2.1e-16, symmetry 8.4e-17, Galerkin 7.4e-8."""
    res = vo.run_case({"case": case, "scale": 8.0})
    assert res["nl"] >= 2 and res["f32"] == 1 and res["coarse_n"] > 0
    assert all(t[2] == "vec" for t in res["table"])
    check(res, case)


def test_f64_transfer_operators(hip, clean_env):
    """HEATFLOW_AMG_F32=0: f64 transfer operators and k_dense_mv; the definition restatement holds to 1e-9.
    Measured: stored 2.9e-16, definition 2.9e-16, Galerkin 6.9e-16, coarse backward error 2.7e-22."""
    clean_env.setenv("HEATFLOW_AMG_F32", "0")
    clean_env.setenv("HEATFLOW_AMG_COARSE", "400")         # (an intermediate level, fused legs in f64)
    res = vo.run_case({"case": "geballe_with_diamond", "scale": 8.0})
    assert res["f32"] == 0 and all(t[5] == "f64" for t in res["table"])
    check(res, "f64")


def test_plain_column_streams(hip, clean_env):
    """HEATFLOW_SPMV_C16=0 (read when a context is created): 32-bit column streams of the fine operator.
    Measured: stored 2.9e-16, definition 1.7e-8."""
    clean_env.setenv("HEATFLOW_SPMV_C16", "0")
    clean_env.setenv("HEATFLOW_AMG_COARSE", "400")
    check(vo.run_case({"case": "geballe_with_diamond", "scale": 8.0}), "c16 off")


def test_coarsest_level_without_dense_inverse(hip, clean_env):
    """A coarsest level beyond 4096 rows has no dense inverse (coarse_n == 0 in the blob): k_scale, w D^-1 b.
    Measured (50323 -> 7772 rows): stored 3.1e-16, definition 3.1e-16."""
    clean_env.setenv("HEATFLOW_AMG_COARSE", "12000")
    res = vo.run_case({"case": "geballe_with_diamond", "scale": 2.0})
    assert res["nl"] >= 2 and res["coarse_n"] == 0 and res["rows"][-1] > 4096, res["rows"]
    check(res, "no coarse inverse")


def test_one_level_hierarchy_on_the_golden_tiny_mesh(hip, clean_env):
    """tests/golden/with_diamond_tiny.npz (1960 nodes): below the coarse size, nl == 1 - two Jacobi sweeps (k_spmv mode 4
    on the fine operator alone).  Measured: stored 9.3e-18, definition 1.5e-16, r.z 0, symmetry 6.4e-17."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "with_diamond_tiny.npz"))
    tags = np.unique(g["tags"])
    with hip.HeatflowHIP(0) as be:
        be.set_mesh(g["coords"], g["tris"], g["tags"])
        be.set_materials(tags, 1.0 + 50.0 * np.arange(len(tags)), 1e6 * (1.0 + np.arange(len(tags))))
        be.set_dirichlet(g["bc_dofs"])
        be.set_precond(hip.PC_AMG, False)
        be.assemble(1e-7, hip.ASM_ROW_GATHER)
        rng = np.random.default_rng(0)
        H, m = vo.check_context(be, {"random": rng.standard_normal(be.n)})
        assert H["header"]["nl"] == 1 and H["header"]["coarse_n"] == 0
        assert m["finite"] and m["bitwise"] and m["stored"] <= STORED and m["definition"] <= 1e-13 and m["rz"] <= RZ, m
        sym, pos = vo.symmetry_and_positivity(lambda x: be.amg_apply(x)[0], be.n)
        assert sym <= 1e-12 and pos > 0.0
        print(f"MEASURED tiny: stored {m['stored']:.2e} definition {m['definition']:.2e} rz {m['rz']:.2e} symmetry {sym:.2e}")


@pytest.mark.parametrize("fuse0", [0, 1, 2])
def test_finest_level_forms_through_the_stream_kernel(hip, tmp_path, fuse0):
    """HEATFLOW_AMG_FUSE0 = 0 / 1 / 2 with HEATFLOW_STREAM_MIN_ROWS=1000: explicit sweeps, both legs fused (GP_0 with
    the r.z epilogue, mode 7) and the fused down leg alone (Rt_0, mode 0) through the LDS-staged kernel.
    Measured: stored <= 2.9e-16, definition <= 4.9e-8 (FUSE0=1), symmetry <= 1.1e-9 (FUSE0=2: the f32 down leg against
    the explicit up leg)."""
    res = child({"case": "geballe_with_diamond", "scale": 8.0}, {"HEATFLOW_AMG_FUSE0": str(fuse0), "HEATFLOW_STREAM_MIN_ROWS": "1000",
                                                           "HEATFLOW_AMG_COARSE": "400"}, tmp_path, f"fuse{fuse0}")
    assert res["fuse0"] == fuse0
    assert bool(streamed(res, 0, "Rt")) == (fuse0 != 0) and bool(streamed(res, 0, "GP")) == (fuse0 == 1), res["table"]
    check(res, f"FUSE0={fuse0}")


@pytest.mark.parametrize("nnz", [700, 6500])
def test_chunk_pipeline_limits(hip, tmp_path, nnz):
    """HEATFLOW_STREAM_NNZ = 700 (many chunks per workgroup, ragged ends, UN = 4) and 6500 (longer chunks, UN = 8 on
    level 1) at mesh scale 2, at least three operators streamed; the UN choice is restated from the blob records
    (vcycle_oracle.stream_pipeline).  No chunk here is longer than UN * TS entries: the second, unpipelined pass is
    reached (and asserted) by the C3 case's GP_1.  Measured pipelines: 700 -> P_0, P_1 at UN 4; 6500 -> P_0 at UN 4,
    P_1 and GP_1 at UN 8.
    Measured: stored 5.8e-16, definition <= 4.9e-8, r.z <= 7.8e-16, symmetry <= 3.3e-10."""
    res = child({"case": "geballe_with_diamond", "scale": 2.0, "install": True},
                {"HEATFLOW_STREAM_MIN_ROWS": "300", "HEATFLOW_STREAM_NNZ": str(nnz)}, tmp_path, f"nnz{nnz}")
    assert len([t for t in res["table"] if t[2] == "stream"]) >= 3, res["table"]
    pipe = res["pipeline"]                               # (level, op, UN, second pass) restated from the blob records
    print(f"MEASURED STREAM_NNZ={nnz}: pipeline {pipe}")
    if nnz == 700:
        assert any(un == 4 for _, _, un, _ in pipe), pipe
    else:
        assert any(un == 8 for _, _, un, _ in pipe), pipe
    # at 700 entries per chunk P_0 has chunks of empty rows (Dirichlet rows without an aggregate): hf_amg_install used
    # to refuse their empty column lists, so the blob of such a hierarchy could not be handed to another context
    assert res["installed"] is True
    check(res, f"STREAM_NNZ={nnz}")


@pytest.mark.parametrize("fuse0", [0, 1, 2])
def test_frozen_hierarchy_after_a_kappa_change(hip, tmp_path, fuse0):
    """hf_update_kappa under reuse = 1: with FUSE0 = 0 / 2 the explicit finest legs run over the NEW operator with the
    old P_0 / R_0; with both legs fused the cycle is that of the OLD operator.
    Measured: stored 2.9e-16, definition <= 4.9e-8 (each against the operator the semantics name)."""
    res = child({"case": "geballe_with_diamond", "scale": 8.0, "reuse": True, "kappa": 1.7},
                {"HEATFLOW_AMG_FUSE0": str(fuse0), "HEATFLOW_STREAM_MIN_ROWS": "1000", "HEATFLOW_AMG_COARSE": "400"},
                tmp_path, f"frozen{fuse0}")
    assert res["stale"] and res["old_operator"] == (fuse0 == 1)
    check(res, f"frozen FUSE0={fuse0}")


def test_c3_default_hierarchy_at_scale(hip, clean_env):
    """The production configuration with default knobs, built as test_gpu_fullsize.py builds C3 (~1.04M DOF): the
    finest level with its fused down leg chosen by size (FUSE0 = 2), the operators through the LDS-staged kernel with the
    default chunking and UN choice, and the real ~1634-row coarse inverse (k_dense_mv_f32).
    Measured (rows 1039371 / 162595 / 16166 / 1634): stored 7.2e-16, definition 7.1e-8, r.z 8.0e-16, symmetry 5.6e-10,
    Galerkin 8.9e-8, coarse backward error 8.0e-22; pipeline P_0 UN 4, Rt_0 UN 8, P_1 UN 8, GP_1 UN 4 with the second pass."""
    res = vo.run_case({"case": "geballe_with_diamond", "scale": 0.43})
    print(f"MEASURED C3: pipeline {res['pipeline']}")
    assert abs(res["n"] - 1.0e6) <= 0.05e6 and res["fuse0"] == 2 and res["f32"] == 1
    assert 1400 <= res["coarse_n"] <= 1900 and res["rows"][-1] == res["coarse_n"], res["rows"]
    assert streamed(res, 0, "Rt") and not any(t[0] == 0 and t[1] == "GP" for t in res["table"]), res["table"]
    assert len([t for t in res["table"] if t[2] == "stream"]) >= 3, res["table"]
    pipe = res["pipeline"]          # (level, op, UN, second pass): both UN choices and the second, unpipelined pass
    assert {un for _, _, un, _ in pipe} == {4, 8} and any(sp2 for _, _, _, sp2 in pipe), pipe
    check(res, "C3")


def test_bdf2_operator_hierarchy(hip, clean_env):
    """Under BDF2 the hierarchy is that of A' = M + 2/3 dt K.  Measured: stored 2.7e-16, definition 1.4e-8."""
    clean_env.setenv("HEATFLOW_AMG_COARSE", "400")
    check(vo.run_case({"case": "geballe_with_diamond", "scale": 8.0, "scheme": "bdf2"}), "bdf2")


def test_perturbed_install_is_caught_and_named(hip, clean_env, case_with_diamond_small):
    """One stored value scaled by (1 + 1e-6) - the largest entry of Rt_1, or of the coarse inverse - and installed with
    hf_amg_install: the device cycle no longer matches the stored-operator restatement of the unperturbed blob (by far
    more than STORED, and by more than 1e3 times the unperturbed error on the same smooth r).  The failure is located from
    that comparison itself (vcycle_oracle.locate): of the stored restatements with one operator of the hierarchy taken from
    the perturbed blob, only the one with the perturbed operator comes back within STORED of the device result.  The
    exported hierarchy of the perturbed context names the same operator (install / export round trip).
    Measured (smooth r): level 1 Rt 3.2e-11, coarse inverse 9.8e-11, against 2.1e-16 unperturbed."""
    from helpers import make_problem

    clean_env.setenv("HEATFLOW_AMG_COARSE", "400")          # an intermediate level with a fused down leg Rt_1
    cfg, stack, mesh = case_with_diamond_small
    base = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True)
    try:
        blob = base.backend.amg_export()
        H = amg_blob.parse(blob)
        A0, d0 = vo.fine_operator(base.backend)
        r = np.ones(A0.shape[0])                                # smooth: the coarse correction carries much of z
        zs = vo.stored_cycle(H, A0, d0, r)
        noise = vo.rel_max(base.backend.amg_apply(r)[0], zs)
    finally:
        base.close()
    assert H["header"]["nl"] >= 3
    rt1 = H["levels"][1]["Rt"]
    for name, entry, want in (("Rt", int(np.argmax(np.abs(rt1.M.data))), "level 1 Rt"),
                              ("inv", int(np.argmax(np.abs(H["coarse_inv"]))), "coarse inverse")):
        bad = amg_blob.perturbed(blob, H, 1, name, entry, 1.0 + 1e-6)
        H_bad = amg_blob.parse(bad)
        prob = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True, amg=bad)
        try:
            z, _ = prob.backend.amg_apply(r)
            err = vo.rel_max(z, zs)
            named = vo.differing_operators(H, vo.parse_export(prob.backend))
        finally:
            prob.close()
        assert err > STORED and err > 1e3 * noise, (want, err, noise)
        print(f"MEASURED perturbed {want}: {err:.2e} against {noise:.2e} unperturbed")
        assert vo.locate(z, H, H_bad, A0, d0, r, STORED) == [want], (want, "cycle against the swapped restatements")
        assert named == [want], named


# ---------------------------------------------------------------------------------------------------------------------
def _batch_columns(hip, case, nv, kind):
    """Batched cycle of nv columns against the per-column stored restatement (finest level explicit, coarse levels
    shared); OP_SHARED also against hf_amg_apply on the same r.  Returns the worst relative error and the columns per
    lane of every operator the batched cycle runs through blaunch_csr (nv: kb_csr, fewer: kb_csr_rc)."""
    from helpers import make_problem, material_tables

    cfg, stack, mesh = case
    prob = make_problem(cfg, stack, mesh, precond=1, amg_reuse=True)
    try:
        be = prob.backend
        H = vo.parse_export(be)
        tag_to_k, _ = material_tables(stack, mesh)
        tag = mesh.material_tags["p_sample"]
        k0 = tag_to_k[tag]
        deltas = k0 * (0.1 * np.arange(nv) - 0.3)
        rng = np.random.default_rng(nv + 10 * kind)
        R = rng.standard_normal((nv, be.n))
        ops = []
        if kind == hip.BATCH_SHARED:
            A0, d0 = vo.fine_operator(be)
            ops = [(A0, d0)] * nv
            be.batch_begin(nv, kind)
        elif kind == hip.BATCH_PER_COLUMN:
            be.batch_begin(nv, kind)
            for j in range(nv):
                be.update_kappa([tag], [k0 * (1.0 + 0.25 * j)])
                ops.append(vo.fine_operator(be))
                be.batch_load_column(j)
        else:
            for j in range(nv):                    # single-path re-assembly at kappa + delta_j
                be.update_kappa([tag], [k0 + deltas[j]])
                ops.append(vo.fine_operator(be))
            be.update_kappa([tag], [k0])
            be.batch_begin(nv, kind)
            be.batch_set_affine([tag], deltas)
        Z, rz = be.batch_apply_precond(R)
        Z2, rz2 = be.batch_apply_precond(R)
        assert np.array_equal(Z, Z2) and np.array_equal(rz, rz2) and np.isfinite(Z).all()
        worst = 0.0
        for j in range(nv):
            zs = vo.stored_cycle(H, ops[j][0], ops[j][1], R[j], explicit=True)
            worst = max(worst, vo.rel_max(Z[j], zs))
            assert abs(rz[j] - R[j] @ Z[j]) <= RZ * np.abs(R[j] * Z[j]).sum(), (j, rz[j], R[j] @ Z[j])
        if kind == hip.BATCH_SHARED:
            be.batch_end()
            for j in range(nv):
                z1, _ = be.amg_apply(R[j])
                worst = max(worst, vo.rel_max(Z[j], z1))
        else:
            be.batch_end()
        L = H["levels"]
        ops = [L[0]["R"], L[0]["P"]] + [L[l][k] for l in range(1, len(L) - 1) for k in ("Rt", "GP")]
        return worst, [vo.batch_columns_per_lane(nv, op) for op in ops]
    finally:
        prob.close()


@pytest.mark.parametrize("nv", [2, 4, 8, 16])
def test_batched_cycle_per_column(hip, clean_env, case_with_diamond_small, nv):
    """kb_csr / kb_csr_rc on the transfer operators, kb_dense<NV, float> on the coarsest level, per-column D^-1:
    OP_SHARED, OP_PERCOL and OP_AFFINE columns against their restatements.  kb_csr_rc (4 columns per lane) is reached
    at nv = 8 and 16 by P_0 (5717 rows), kb_csr by every other launch.  Measured worst column: nv 2 3.4e-16, nv 4 4.0e-16, nv 8 5.0e-16,
    nv 16 5.8e-16."""
    for kind in (hip.BATCH_SHARED, hip.BATCH_PER_COLUMN, hip.BATCH_AFFINE):
        worst, cpl = _batch_columns(hip, case_with_diamond_small, nv, kind)
        print(f"MEASURED batched nv={nv} kind={kind}: {worst:.2e} columns per lane {cpl}")
        assert worst <= STORED, (nv, kind, worst)
        assert (min(cpl) < nv) == (nv >= 8), (nv, cpl)


def test_batched_dense_rows_per_column_split(hip, tmp_path):
    """HEATFLOW_BATCH_DENSE_CPL=1 (read once): kb_dense_rc on the coarsest level.  Measured: 4.0e-16."""
    script = tmp_path / "dense_cpl.py"
    script.write_text(
        "import sys\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "from conftest import build_case\n"
        "from heatflow_amd import hip_backend as hip\n"
        "import test_gpu_vcycle as t\n"
        "case = build_case('geballe_with_diamond', 8.0)\n"
        "w = max(t._batch_columns(hip, case, nv, k)[0] for nv in (4, 16) for k in (hip.BATCH_SHARED, hip.BATCH_AFFINE))\n"
        "print('WORST', w)\n")
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env["HEATFLOW_BATCH_DENSE_CPL"] = "1"
    res = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    worst = float(res.stdout.split("WORST")[-1])
    print(f"MEASURED dense cpl: {worst:.2e}")
    assert worst <= STORED, worst


# ---------------------------------------------------------------------------------------------------------------------
def _spd(kind, n, rng):
    if kind.startswith("dense"):
        cond = 1e2 if kind == "dense1e2" else 1e8
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        ev = np.logspace(0, np.log10(cond), n)
        S = (Q * ev) @ Q.T
        return sp.csr_matrix((S + S.T) / 2)
    # 2-D P1-like 5-point operator with the stack's contrast (kappa 2000 against 3.8, rho_c ratio ~10), rows scaled
    # over six decades (symmetric diagonal scaling), optionally with eliminated (unit) rows, one at a block boundary
    nx = int(np.ceil(np.sqrt(n)))
    ii = np.arange(n)
    x, y = ii % nx, ii // nx
    kap = np.where(x < nx // 2, 2000.0, 3.8)
    rc = np.where(y % 2 == 0, 1.0, 10.0)
    rows, cols, vals = [], [], []
    diag = 0.05 * rc.copy()
    for di, ok in ((1, x + 1 < nx), (nx, ii + nx < n)):
        a = ii[ok & (ii + di < n)]
        b = a + di
        k = np.sqrt(kap[a] * kap[b])
        rows += [a, b]
        cols += [b, a]
        vals += [-k, -k]
        np.add.at(diag, a, k)
        np.add.at(diag, b, k)
    S = sp.csr_matrix((np.concatenate(vals + [diag]), (np.concatenate(rows + [ii]), np.concatenate(cols + [ii]))), shape=(n, n))
    s = np.logspace(-3, 3, n)[rng.permutation(n)]
    S = sp.diags(s) @ S @ sp.diags(s)
    if kind == "p1_dirichlet" and n >= 4:
        unit = set(range(1, n, 7)) | ({32 * (n // 64)} if n > 64 else set())
        keep = np.array([0.0 if i in unit else 1.0 for i in range(n)])
        D = sp.diags(keep)
        S = D @ S @ D + sp.diags(1.0 - keep)
    return sp.csr_matrix(S)


DENSE_N = [1, 2, 3, 31, 32, 33, 63, 64, 65, 97, 255, 256, 257, 1634, 2047, 4095, 4096]


@pytest.mark.parametrize("kind", ["dense1e2", "dense1e8", "p1", "p1_dirichlet"])
def test_dense_inverse_at_the_edges(hip, kind):
    """hf_dense_inverse: the blocked Gauss-Jordan inverse (k_gjb_fill / k_gjb_rows / k_gjb_update) at tail blocks
    (n mod 32), tile edges (n mod 64) and the 4096-row limit, and k_dense_mv / k_dense_mv_f32 at odd n and n mod 4 != 0
    (half-row pairing, pad columns).
      backward error  ||S X - I||_max <= 1e-10 ||S|| ||X||
      forward error   against numpy.linalg.inv, max|X - X_ref| / max|X_ref|:
                      dense kinds: <= 1e3 cond(S) eps (inf-norm condition; the bound is asserted to be below 1);
                      row-scaled P1 kinds: cond(S) passes 1e13 there, so that bound is >= 1 and could not fail.  They
                      are measured in the symmetrically equilibrated form (D X D, D = diag(S)^1/2, whose condition does
                      not depend on the row scaling) against max(1e3, 10 n) cond(D^-1 S D^-1) eps, below 1e-9 at every n.
      products        each row of k_dense_mv to 1e-13 of (|X| |b|) for that row, k_dense_mv_f32 likewise on float(X).
    Measured worst over n (backward error / forward error as a fraction of its bound / k_dense_mv / k_dense_mv_f32 row
    error): dense 1e2 4.1e-17 / 5.8e-5 / 2.1e-16 / 1.7e-16; dense 1e8 7.3e-13 / 0.98 / 1.6e-16 / 1.6e-16 (inf-norm
    condition 8.8e9; the numpy reference's own error is of the same order there); P1 1.3e-22 / 1.3e-3 / 1.3e-15 /
    1.3e-15; P1 with unit rows 1.3e-22 / 0.11 / 2.8e-15 / 1.8e-15."""
    rng = np.random.default_rng(7)
    eps = np.finfo(np.float64).eps
    worst = {"back": 0.0, "fwd/bound": 0.0, "x64": 0.0, "x32": 0.0, "cond_eq": 0.0}
    with hip.HeatflowHIP(0) as be:
        for n in DENSE_N:
            S = _spd(kind, n, rng)
            b = rng.standard_normal(n)
            X, x64, x32 = be.dense_inverse(S, b)
            Sd = S.toarray()
            nS, nX = np.abs(Sd).sum(1).max(), np.abs(X).sum(1).max()
            back = np.abs(Sd @ X - np.eye(n)).max() / (nS * nX)
            assert back <= 1e-10, (kind, n, back)
            Xr = np.linalg.inv(Sd)
            if kind.startswith("dense"):
                cond_eq = nS * np.abs(Xr).sum(1).max()
                fwd = np.abs(X - Xr).max() / np.abs(Xr).max()
                bound = 1e3 * cond_eq * eps
            else:
                d = np.sqrt(np.diag(Sd))
                Se, Xe, Xre = Sd / np.outer(d, d), X * np.outer(d, d), Xr * np.outer(d, d)
                cond_eq = np.abs(Se).sum(1).max() * np.abs(Xre).sum(1).max()
                fwd = np.abs(Xe - Xre).max() / np.abs(Xre).max()
                bound = max(1e3, 10.0 * n) * cond_eq * eps
            assert bound < 1.0, (kind, n, "a forward-error bound that cannot fail", bound)
            assert fwd <= bound, (kind, n, fwd, cond_eq)
            e64 = np.max(np.abs(x64 - X @ b) / (np.abs(X) @ np.abs(b) + 1e-300))
            assert e64 <= 1e-13, (kind, n, "k_dense_mv", e64)
            Xf = X.astype(np.float32).astype(np.float64)
            e32 = np.max(np.abs(x32 - Xf @ b) / (np.abs(Xf) @ np.abs(b) + 1e-300))
            assert e32 <= 1e-13, (kind, n, "k_dense_mv_f32", e32)
            for k, v in (("back", back), ("fwd/bound", fwd / bound), ("x64", e64), ("x32", e32), ("cond_eq", cond_eq)):
                worst[k] = max(worst[k], float(v))
        print(f"MEASURED dense {kind}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        with pytest.raises(ValueError):
            be.dense_inverse(sp.identity(4097, format="csr"), np.ones(4097))
