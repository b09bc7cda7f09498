"""Picard steady state under kappa(T) / rho_c(T) tables without a GPU: the entry points are declared and exported, the
restatement of tests/steady_picard_oracle.py reproduces the exact solution of a Kirchhoff problem, and
HeatProblem.solve_steady routes to the Picard calls with tables and to the linear calls without."""
import numpy as np

from steady_picard_oracle import picard_steady, rectangle_mesh
from test_cabi import _declared_symbols

NEW_ENTRY_POINTS = ("hf_steady_picard_setup", "hf_steady_picard_solve")


def test_header_declares_and_library_exports_the_picard_steady_entry_points():
    from heatflow_amd import hip_backend

    declared = _declared_symbols()
    lib = hip_backend.load_library()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in hip_backend.EXPORTS, name
        assert hasattr(lib, name), name


# Kirchhoff pin ----------------------------------------------------------------------------------------------------------------
# One material with k(T) = k0 * 300 / T between z = 0 at 300 K and z = L at 900 K, natural elsewhere: the Kirchhoff variable
# theta = int k dT = 300 k0 ln T is harmonic and depends on z alone, so ln T is linear in z and T(z) = 300 * 3^(z / L).
# Only z is refined (the answer does not depend on r): two cells across the radius, their diagonals alternating, so that the
# discrete answer is not the nodally exact one a one-directional triangulation gives for a field of z alone.
def _kirchhoff_error(nz):
    L, R, k0 = 4e-6, 2e-6, 10.0
    coords, tris = rectangle_mesh(nz, 2, L, R)
    tags = np.ones(len(tris), dtype=np.int32)
    knots = 256
    dT = 600.0 / (knots - 1)
    tables = {1: (300.0, dT, k0 * 300.0 / (300.0 + dT * np.arange(knots)))}
    lo = np.flatnonzero(coords[:, 0] == 0.0)
    hi = np.flatnonzero(coords[:, 0] == L)
    dofs = np.concatenate([lo, hi])
    g = np.concatenate([np.full(len(lo), 300.0), np.full(len(hi), 900.0)])
    exact = 300.0 * 3.0 ** (coords[:, 0] / L)
    x0 = np.full(len(coords), 300.0)
    out = picard_steady(coords, tris, tags, {1: k0}, dofs, g, x0, tables, picard_tol=1e-9, max_sweeps=60)
    lin = picard_steady(coords, tris, tags, {1: k0}, dofs, g, x0, None, picard_tol=1e-9, max_sweeps=3)
    assert out["converged"] and lin["converged"] and lin["sweeps"] == 2
    return float(np.abs(out["u"] - exact).max()), float(np.abs(lin["u"] - exact).max()), out


def test_restated_picard_loop_reproduces_the_kirchhoff_solution():
    e32, _, _ = _kirchhoff_error(32)
    e64, lin64, out = _kirchhoff_error(64)
    print(f"Kirchhoff: error {e32:.4f} K at 32 cells, {e64:.4f} K at 64 cells (x{e32 / e64:.2f}); constant k {lin64:.1f} K off; "
          f"{out['sweeps']} sweeps, nl_resid {out['nl_resid']:.2e}")
    assert e64 <= 0.1, e64
    assert e32 / e64 >= 3.5, e32 / e64
    assert lin64 > 50.0                      # the constant-k answer is the straight line: far off
    assert out["nl_resid"] <= 1e-8
    ch = np.array(out["changes"])
    assert np.all(ch[1:] < ch[:-1])          # the iteration contracts monotonically


# routing ------------------------------------------------------------------------------------------------------------------------
class RecordingBackend:
    """Records every call HeatProblem makes; the steady calls answer with recognisable values."""

    def __init__(self):
        self.calls = []
        self.n = 0

    def set_mesh(self, coords, tris, tags, pattern=None):
        self.n = len(coords)
        self.calls.append(("set_mesh",))

    def get_state(self):
        return np.full(self.n, 321.0)

    def steady_solve(self, g, use_load=False, rtol=1e-10, atol=0.0, max_it=20000):
        self.calls.append(("steady_solve", len(g), bool(use_load), rtol, atol, max_it))
        return 17, 2.5e-11

    def steady_picard_solve(self, g, use_load=False, rtol=1e-10, atol=0.0, max_it=20000, picard_tol=1e-6, max_sweeps=50):
        self.calls.append(("steady_picard_solve", len(g), bool(use_load), rtol, atol, max_it, picard_tol, max_sweeps))
        return {"sweeps": 3, "iters": [40, 12, 0], "change": 4e-8, "nl_resid": 3e-9}

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)

        def record(*a, **kw):
            self.calls.append((name,) + tuple(x for x in a if np.isscalar(x)))

        return record


def _problem(case, **kw):
    from heatflow_amd.solver import HeatProblem
    from helpers import material_tables
    from test_steady_cpu import steady_bcs

    cfg, stack, mesh = case
    ic = float(cfg["heating"]["ic_temp"])
    tk, trc = material_tables(stack, mesh)
    sb = steady_bcs(cfg, stack, mesh, ic + 400.0, ic + 250.0)
    be = RecordingBackend()
    prob = HeatProblem(mesh.coords, mesh.tris, mesh.tags, tk, trc, 1e-7, sb[:3], ic, backend=be, rtol=1e-12, max_it=1234, **kw)
    return prob, be, sb, tk, trc


def _names(be):
    return [c[0] for c in be.calls]


def test_solve_steady_takes_the_picard_calls_with_tables_of_either_kind(case_with_diamond_small):
    cfg, stack, mesh = case_with_diamond_small
    tag = mesh.material_tags["p_ins"]
    for which in ("kappa", "rhoc", "both"):
        _, _, _, tk, trc = _problem(case_with_diamond_small)
        kw = {}
        if which in ("kappa", "both"):
            kw["kappa_tables"] = {tag: (300.0, 100.0, [tk[tag], 0.5 * tk[tag]])}
        if which in ("rhoc", "both"):
            kw["rhoc_tables"] = {tag: (300.0, 100.0, [trc[tag], 1.5 * trc[tag]])}
        prob, be, sb, _, _ = _problem(case_with_diamond_small, **kw)
        del be.calls[:]
        u, it, res = prob.solve_steady(sb, picard_tol=1e-7, max_sweeps=9)
        assert _names(be) == ["steady_picard_setup", "steady_picard_solve"], (which, be.calls)
        assert be.calls[0][1:] == (prob.precond,)
        nS = len(np.unique(np.concatenate([b.row_dofs for b in sb])))
        assert be.calls[1] == ("steady_picard_solve", nS, False, 1e-12, 0.0, 1234, 1e-7, 9)
        assert (it, res) == (52, 3e-9) and u.shape == (prob.n,) and np.all(u == 321.0)
        assert prob.steady_info == {"sweeps": 3, "iters": [40, 12, 0], "change": 4e-8, "nl_resid": 3e-9}
        del be.calls[:]
        prob.solve_steady(sb, use_load=True)                       # the defaults of the issue
        assert be.calls[1][2] is True and be.calls[1][6:] == (1e-6, 50)


def test_solve_steady_without_tables_calls_what_it_called_before(case_with_diamond_small):
    prob, be, sb, _, _ = _problem(case_with_diamond_small)
    del be.calls[:]
    u, it, res = prob.solve_steady(sb)
    assert _names(be) == ["steady_setup", "steady_solve"], be.calls
    nS = len(np.unique(np.concatenate([b.row_dofs for b in sb])))
    assert be.calls[1] == ("steady_solve", nS, False, 1e-12, 0.0, 1234)
    assert (it, res) == (17, 2.5e-11) and np.all(u == 321.0)
    assert not hasattr(prob, "steady_info")
