"""-m gpu: multi-term solver equations -- div(u, phi) +- laplacian(nu, phi), grad(phi) - laplacian(eps, phi), one
operator object used twice -- through Solver.set_eq / Aop / solve on every solver path, against the REFERENCE's
recorded runs (goldens of kind "eqn", tests/golden/make_golden.py::run_eqn) and, on meshes too large for fixtures
(the two-term tiling of the 3-D / 2-D kernels), against the oracle those goldens pin
(tests/test_oracle_golden.py::test_oracle_equation).

What only these see: the Div / Grad rhs adjustment on an inhomogeneous Neumann face (its sign, its dependence on the
sign of u and on the face side, per-node Neumann values under a Div term), the order the terms' adjustments are added
in, the + u phi / r row of an axisymmetric Div and a tensor speed inside a solve.  Everything else in the suite that
runs these equations compares one product path with another."""
import warnings

import pytest
import torch

from conftest import golden_cases, golden_load
from helpers import (TILED_EQN_K, bit_equal, eqn_build, eqn_cfg, eqn_inputs, eqn_oracle, hip_options, product_mesh,
                     rel_err, tiled_eqn_cases)

pytestmark = pytest.mark.gpu

from pyapes_amd.hip.context import context_for
from pyapes_amd.solver.fdm import FDM
from pyapes_amd.solver.ops import Solver
from pyapes_amd.variables import Field

OPTIONS = ("fastpath", "resident", "fold", "rhs_full")


def _set_eq(monkeypatch, case, x0, rhs0, tensor, K, **opts):
    """A fresh mesh (its context takes the options when it is created), the field at x0, the equation set.
    -> (solver, var, the rhs handed to set_eq (None: a float), mesh)"""
    hip_options(monkeypatch, **{k: opts.get(k) for k in OPTIONS})
    mesh = product_mesh(case)
    cfg = [dict(c, bc_val_opt=None) for c in eqn_cfg(case)]
    var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
    var.set_var_tensor(torch.as_tensor(x0).cuda().clone())
    fcfg = None
    if "limiter" in case:   # the reference's literal upwind is the product's compat form
        fcfg = {"div": {"limiter": case["limiter"], "edge": False, "compat": case["limiter"] == "upwind"}}
    s = Solver({"fdm": {"method": case["method"], "tol": case["tol"], "max_it": K, "report": False}})
    rhs = None if "rhs_float" in case else torch.as_tensor(rhs0).cuda().clone()
    eq = eqn_build(FDM(fcfg), var, case, torch.as_tensor(tensor).cuda())
    s.set_eq(eq == (case["rhs_float"] if rhs is None else rhs))
    return s, var, rhs, mesh


def _solve(s):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return s.solve()


def _check_rhs(monkeypatch, case, x0, rhs0, tensor, want):
    for full in (0, 1):
        s, _, rhs, _ = _set_eq(monkeypatch, case, x0, rhs0, tensor, 1, rhs_full=full)
        assert bit_equal(s.rhs, want), (case["name"], "rhs after set_eq", full, float((s.rhs.cpu() - want).abs().max()))
        if rhs is not None:
            assert bit_equal(rhs, want), "set_eq must modify the caller's rhs in place (Q9)"


def _check_aop(monkeypatch, case, x0, rhs0, tensor, want):
    for fast in (0, 1):
        s, var, _, _ = _set_eq(monkeypatch, case, x0, rhs0, tensor, 1, fastpath=fast)
        var.apply_bcs()
        ax = s.Aop(var)
        assert bit_equal(ax, want), (case["name"], "Aop", fast, float((ax.cpu() - want).abs().max()))


EQN = golden_cases("eqn")


@pytest.mark.parametrize("case", EQN, ids=lambda c: c["name"])
def test_rhs_after_set_eq_bit_exact(case, monkeypatch):
    """solver.rhs = the reference's, bit for bit: every term's adjustment, unsigned, in term order; the caller's
    tensor modified in place; the layer kernel and the whole-mesh one (option rhs_full)"""
    g = golden_load(case["name"])
    want = torch.from_numpy(g["rhs_set_eq"])
    neumann = case["bcs"] == "pernode3d" or any(t == "neumann" for t, _ in case["bcs"])
    assert torch.equal(want, torch.from_numpy(g["rhs0"])) != neumann   # the fixture's adjustment is not zero
    _check_rhs(monkeypatch, case, g["x0"], g["rhs0"], g["u_tensor"], want)


@pytest.mark.parametrize("case", EQN, ids=lambda c: c["name"])
def test_aop_bit_exact(case, monkeypatch):
    """solver.Aop on the BC-filled x0 = the reference's, bit for bit, tiled and generic kernels"""
    g = golden_load(case["name"])
    _check_aop(monkeypatch, case, g["x0"], g["rhs0"], g["u_tensor"], torch.from_numpy(g["aop"]))


# the meshes whose resident=1 solves must run the resident loop (the general-equation build of pa_resident.hip): with a
# plan of 0 workgroups the sweep below would compare the launch-per-phase loop with itself
MUST_RUN_RESIDENT = ("eqn2d_mix", "eqn3d_mix", "eqn_rz_mix")


@pytest.mark.parametrize("case", EQN, ids=lambda c: c["name"])
def test_solve_vs_reference_every_path(case, monkeypatch):
    """iterates and reports of the reference's recorded runs on fastpath x resident x fold: identical counts, 1e-10
    rel (fp32: 1e-5) -- the bar of test_gpu_parity_golden.py::test_solve_vs_reference for short fixed counts --
    and rep["tol"] to 1e-6 rel in fp64.  Where the plan takes the mesh, resident=1 must have run resident."""
    g = golden_load(case["name"])
    rtol = 1e-10 if case["dtype"] == "double" else 1e-5
    for fast in (0, 1):
        for resident in (0, 1):
            for fold in (0, 1):
                for K in case["max_its"]:
                    ref = g["_reports"][str(K)]
                    s, var, _, mesh = _set_eq(monkeypatch, case, g["x0"], g["rhs0"], g["u_tensor"], K, fastpath=fast,
                                              resident=resident, fold=fold)
                    rep = _solve(s)
                    where = (case["name"], K, fast, resident, fold)
                    ctx = context_for(mesh)
                    used, plan = ctx.resident_used(), ctx.resident_plan(case["method"])[0]
                    assert used == (plan if resident else 0), (where, used, plan)
                    if resident and case["name"].startswith(MUST_RUN_RESIDENT):
                        assert used > 0, (where, used, plan)
                    assert rep["itr"] == ref["itr"] and rep["converge"] == ref["converge"], (where, rep, ref)
                    err = rel_err(var().cpu(), g[f"x_K{K}"])
                    assert err <= rtol, (where, err)
                    if case["dtype"] == "double":
                        assert abs(rep["tol"] - ref["tol"]) <= 1e-6 * abs(ref["tol"]), (where, rep, ref)


# ---- the tiled two-term kernels against the oracle ---------------------------------------------------------------
TILED = tiled_eqn_cases()


@pytest.mark.parametrize("case", TILED, ids=lambda c: c["name"])
def test_tiled_equation_vs_oracle(case, monkeypatch):
    """whole rows, more than one k tile, pitched rows, 2-D, fp32: rhs after set_eq and A x bit for bit, 3 BiCGSTAB
    iterations from a random x0 to 1e-9 (fp32: 5e-5; the bars of test_gpu_fuzz.py::test_seeded_fuzz_bicgstab) with the
    oracle's counts, tiled (fastpath 1) and generic (0) launch-per-phase kernels.  The tensor speed runs the generic
    kernels either way."""
    x0, rhs0, ut = eqn_inputs(case)
    rhs_o, ax_o, x_o, rep_o = eqn_oracle(case, x0, rhs0, ut, TILED_EQN_K)
    _check_rhs(monkeypatch, case, x0, rhs0, ut, rhs_o)
    _check_aop(monkeypatch, case, x0, rhs0, ut, ax_o)
    rtol = 1e-9 if case["dtype"] == "double" else 5e-5
    for fast in (1, 0):
        s, var, _, mesh = _set_eq(monkeypatch, case, x0, rhs0, ut, TILED_EQN_K, fastpath=fast, resident=0)
        rep = _solve(s)
        assert context_for(mesh).resident_used() == 0
        assert rep["itr"] == rep_o["itr"] == TILED_EQN_K and rep["converge"] == rep_o["converge"], (fast, rep, rep_o)
        err = rel_err(var().cpu(), x_o)
        assert err <= rtol, (case["name"], fast, err)
