"""-m gpu: the folded launch sequence (scalar steps in the prologue of the next tiled kernel, DESIGN.md §4 "small meshes") against the launch sequence it replaces
(PYAPES_HIP_FOLD=0): same bits in the iterate, same iteration count, same
tolerance -- for CG, Jacobi and BiCGSTAB, dozens of iterations (so that batches, polls and the flush of a
pending step all happen), random extents / face types / dtypes, and a stop inside a batch."""
import os
import random
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

from pyapes_amd.geometry import Box
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdm import FDM
from pyapes_amd.solver.ops import Solver
from pyapes_amd.variables import Field

def _faces():
    import pyapes_oracle as O
    return O.FACES


def _solve(monkeypatch, folded, n, bcs, dtype, method, rhs, x0, tol, max_it, adv):
    monkeypatch.setenv("PYAPES_HIP_FOLD", "1" if folded else "0")
    nd = len(n)
    mesh = Mesh(Box([0.0] * nd, [1.0 + 0.1 * a for a in range(nd)]), None, list(n), "cuda", dtype)
    cfg = [{"bc_face": _faces()[i], "bc_type": t, "bc_val": v, "bc_val_opt": None} for i, (t, v) in enumerate(bcs)]
    var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
    var.set_var_tensor(x0.cuda().clone())
    s = Solver({"fdm": {"method": method, "tol": tol, "max_it": max_it, "report": False}})
    fdm = FDM({"div": {"limiter": "upwind", "edge": False}})
    if adv:
        s.set_eq(fdm.div(0.6, var) - fdm.laplacian(0.05, var) == rhs.cuda().clone())
    else:
        s.set_eq(-fdm.laplacian(0.8, var) == rhs.cuda().clone())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = s.solve()
    return var().cpu(), rep


def _case(rng):
    nd = rng.choice([2, 3, 3])
    if nd == 2:
        n = [rng.choice([9, 16, 33, 64, 100, 129]), rng.choice([8, 17, 64, 65, 128, 130])]
    else:
        n = [rng.choice([5, 8, 12, 17, 24, 33]), rng.choice([6, 9, 16, 20, 40]), rng.choice([8, 17, 32, 33, 64, 66])]
    bcs = []
    for a in range(nd):
        if rng.random() < 0.2:
            bcs += [("periodic", None), ("periodic", None)]
        else:
            for _ in range(2):
                t = rng.choice(["dirichlet", "dirichlet", "neumann", "symmetry"])
                bcs.append((t, None if t == "symmetry" else round(rng.uniform(-1, 1), 3)))
    if not any(t == "dirichlet" for t, _ in bcs):
        bcs[0] = ("dirichlet", 0.25)
        if bcs[1][0] == "periodic":
            bcs[1] = ("dirichlet", -0.5)
    dtype = "double" if rng.random() < 0.7 else "single"
    return n, bcs, dtype


@pytest.mark.parametrize("method", ["cg", "jacobi", "bicgstab"])
def test_folded_sequence_is_bit_identical(monkeypatch, method):
    ncases = int(os.environ.get("PYAPES_FUZZ_CASES", "40"))   # soak runs: PYAPES_FUZZ_CASES=1000
    rng = random.Random(7 + len(method) + ncases)
    checked = 0
    for case in range(ncases):
        n, bcs, dtype = _case(rng)
        tdt = torch.float64 if dtype == "double" else torch.float32
        g = torch.Generator().manual_seed(1000 + case)
        rhs = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        x0 = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        adv = method == "bicgstab" and case % 2 == 0
        # every third case stops on the tolerance somewhere inside a batch of enqueued iterations
        tol = -1.0 if case % 3 else (1e-3 if dtype == "double" else 1e-2)
        max_it = 37 if case % 3 else 400
        try:
            xa, ra = _solve(monkeypatch, True, n, bcs, dtype, method, rhs, x0, tol, max_it, adv)
        except RuntimeError:
            with pytest.raises(RuntimeError):   # non-finite stop test: both sequences must raise
                _solve(monkeypatch, False, n, bcs, dtype, method, rhs, x0, tol, max_it, adv)
            continue
        xb, rb = _solve(monkeypatch, False, n, bcs, dtype, method, rhs, x0, tol, max_it, adv)
        assert ra["itr"] == rb["itr"], (case, n, bcs, dtype, ra, rb)
        assert ra["tol"] == rb["tol"] or (ra["tol"] != ra["tol"] and rb["tol"] != rb["tol"]), (case, n, bcs, ra, rb)
        assert torch.equal(xa, xb), (case, n, bcs, dtype, float((xa - xb).abs().max()))
        checked += 1
    assert checked >= ncases // 2


# ---- every folded prologue against the unfolded sequence, bit for bit, on ALL the scalars -----------------------------
# One mesh per prologue that exists (k_cg3d: vector / narrow / pitched layout; k_cg2d: plain, pitched, fp32, periodic
# slow axis, axisymmetric), at the smallest shape the launch conditions admit (launch_cg2d: n1 >= 8, n2 >= 2 vectors;
# solver_pitch).  test_every_prologue_case_runs_the_kernel_it_names reads the launch log of the same cases.
_DD = [("dirichlet", 0.25), ("dirichlet", -0.5)]
_DN = [("dirichlet", 0.25), ("neumann", 0.1)]
_PE = [("periodic", None), ("periodic", None)]
PROLOGUE_CASES = {
    # name: (n, dtype, faces, options, geometry, kernel, layout tag of the launch log)
    "cg2d_pitched_f64": ([9, 21], "double", _DN + _DD, {"cg2d_mincells": 0, "pitch": 1}, "box", "k_cg2d", " (pitched)"),
    "cg2d_f64": ([12, 40], "double", _DD + _DN, {"cg2d_mincells": 0}, "box", "k_cg2d", ""),
    "cg2d_f32": ([10, 24], "single", _DD + _DN, {"cg2d_mincells": 0}, "box", "k_cg2d", ""),
    "cg2d_slow_periodic_f64": ([8, 16], "double", _PE + _DD, {"cg2d_mincells": 0}, "box", "k_cg2d", ""),
    "cg2d_rz_f64": ([12, 40], "double", [("neumann", 0.0), ("dirichlet", 1.0), ("dirichlet", 0.3), ("neumann", 0.5)],
                    {"cg2d_mincells": 0}, "cylinder", "k_cg2d", ""),
    "cg3d_vector_f64": ([6, 12, 16], "double", _DD + _DN + _DD, {}, "box", "k_cg3d", ""),
    "cg3d_vector_f32": ([6, 12, 16], "single", _DD + _DN + _DD, {}, "box", "k_cg3d", ""),
    "cg3d_narrow_f64": ([6, 9, 13], "double", _DD + _DN + _DD, {"pitch": 0}, "box", "k_cg3d", " (narrow)"),
    "cg3d_pitched_f64": ([6, 9, 13], "double", _DD + _DN + _DD, {"pitch": 1}, "box", "k_cg3d", " (pitched)"),
}


def _prologue_methods(name):
    return ("cg", "bicgstab") if "rz" in name else ("cg", "jacobi", "bicgstab")


def _prologue_solve(name, method, fold, tol, max_it):
    from pyapes_amd.geometry import Cylinder
    from pyapes_amd.hip.context import context_for
    n, dtype, faces, options, geometry, _, _ = PROLOGUE_CASES[name]
    nd = len(n)
    hi = [1.0 + 0.1 * a for a in range(nd)]
    mesh = Mesh(Cylinder([0.0] * nd, hi) if geometry == "cylinder" else Box([0.0] * nd, hi), None, list(n), "cuda", dtype)
    ctx = context_for(mesh)
    ctx.set_option("resident", 0)
    ctx.set_option("fold", fold)
    for k, v in options.items():
        ctx.set_option(k, v)
    import pyapes_oracle as O
    names = O.FACES_RZ if geometry == "cylinder" else O.FACES
    # (data of size 1e-6: the stop test of the first iteration is `1.0 > tolerance`, so a tolerance taken from the run
    # itself has to be below 1)
    cfg = [{"bc_face": names[i], "bc_type": t, "bc_val": None if v is None else 1e-6 * v, "bc_val_opt": None}
           for i, (t, v) in enumerate(faces)]
    var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
    g = torch.Generator().manual_seed(5)
    tdt = torch.float64 if dtype == "double" else torch.float32
    rhs = (1e-6 * torch.randn((1, *n), generator=g, dtype=torch.float64)).to(tdt)
    var.set_var_tensor((1e-6 * torch.randn((1, *n), generator=g, dtype=torch.float64)).to(tdt).cuda())
    s = Solver({"fdm": {"method": method, "tol": tol, "max_it": max_it, "report": False}})
    s.set_eq(-FDM().laplacian(0.8, var) == rhs.cuda())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = s.solve()
    return var().cpu(), rep, ctx.scalars()


def _same(a, b):
    return a == b or (a != a and b != b)


@pytest.mark.parametrize("method", ["cg", "jacobi", "bicgstab"])
def test_folded_scalars_equal_on_every_prologue(method):
    """fold 1 against fold 0: the iterate, the iteration count, tol and EVERY entry of ctx.scalars(), bit for bit --
    K = 7 iterations with tol = -1, and once with a tolerance that stops inside the run (the value the unfolded
    sequence reports after three iterations: `tol <= tolerance` holds there at the latest)."""
    K = 7
    for name in PROLOGUE_CASES:
        if method not in _prologue_methods(name):
            continue
        _, r3, _ = _prologue_solve(name, method, 0, -1.0, 3 if method == "bicgstab" else 2)
        assert r3["itr"] == 3 and 0.0 < r3["tol"] < 1.0, (name, r3)
        for tol in (-1.0, r3["tol"]):
            xa, ra, sa = _prologue_solve(name, method, 1, tol, K)
            xb, rb, sb = _prologue_solve(name, method, 0, tol, K)
            assert torch.equal(xa, xb), (name, tol, float((xa - xb).abs().max()))
            assert ra["itr"] == rb["itr"], (name, tol, ra, rb)
            assert _same(ra["tol"], rb["tol"]), (name, tol, ra, rb)
            assert set(sa) == set(sb) and len(sa) == 14
            for key in sb:
                assert _same(sa[key], sb[key]), (name, tol, key, sa[key], sb[key])
            full = K if method == "bicgstab" else K + 1   # (`itr >= max_it` against `itr > max_it`)
            assert rb["itr"] == full if tol < 0 else 1 <= rb["itr"] <= 3, (name, tol, rb)
            if tol < 0:
                sk = sa
        # the last beta of the K-iteration run, restated from the scalars it was formed from in the mesh's precision
        # and the reference's order (linalg.py:141: r'.r' / r.r; linalg.py:212: rho' / rho * alpha / omega, rho = the rho
        # one iteration earlier): fold 1 and fold 0 run the SAME step function, so their agreement alone does not pin it
        import numpy as np
        f = np.float64 if PROLOGUE_CASES[name][1] == "double" else np.float32
        if method == "cg":
            assert sk["beta"] == float(f(sk["rr"]) / f(sk["rr_old"])), (name, sk)
            assert sk["alpha"] == float(f(sk["rr_old"]) / f(sk["dAd"])), (name, sk)
        if method == "bicgstab":
            _, _, sp = _prologue_solve(name, method, 0, -1.0, K - 1)
            beta = f(sk["rho_next"]) / f(sp["rho"])
            beta = beta * f(sk["alpha"])
            beta = beta / f(sk["omega"])
            assert sk["beta"] == float(beta) and sk["rho"] == sk["rho_next"], (name, sk, sp)


# The Jacobi sweep with a coefficient FIELD, fp32, odd rows (one cell per lane), at most 4 rows (one row per thread):
# k_cg3d<float, 1, 4 | 9, CF, 0, NARROW>, the instantiation whose grid launch_cg3d holds at 6 blocks / CU.  More planes than
# 6 x CUs, so that the chunks -- and with them the grouping of |dx|^2 -- follow that figure and not the mesh.
CF_JACOBI_N = [1600, 4, 13]


def _cf_jacobi_solve(fold, max_it):
    from pyapes_amd.hip.context import context_for
    n = CF_JACOBI_N
    mesh = Mesh(Box([0.0] * 3, [1.0, 1.1, 1.2]), None, list(n), "cuda", "single")
    ctx = context_for(mesh)
    ctx.set_option("resident", 0)
    ctx.set_option("fold", fold)
    cfg = [{"bc_face": _faces()[i], "bc_type": t, "bc_val": v, "bc_val_opt": None} for i, (t, v) in enumerate(_DD + _DN + _DD)]
    var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
    g = torch.Generator().manual_seed(6)
    rhs = torch.randn((1, *n), generator=g, dtype=torch.float64).float()
    var.set_var_tensor(torch.randn((1, *n), generator=g, dtype=torch.float64).float().cuda())
    gamma = (1.0 + 0.2 * torch.rand((1, *n), generator=g, dtype=torch.float64)).float()
    s = Solver({"fdm": {"method": "jacobi", "tol": -1.0, "max_it": max_it, "report": False}})
    s.set_eq(-FDM().laplacian(gamma.cuda(), var) == rhs.cuda())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = s.solve()
    return var().cpu(), rep, ctx.scalars()


def test_folded_scalars_equal_on_the_coefficient_field_sweep():
    """fold 1 against fold 0 on that instantiation: iterate, iteration count, tol and every scalar, bit for bit"""
    xa, ra, sa = _cf_jacobi_solve(1, 7)
    xb, rb, sb = _cf_jacobi_solve(0, 7)
    assert torch.equal(xa, xb) and ra["itr"] == rb["itr"] == 8 and _same(ra["tol"], rb["tol"]), (ra, rb)
    assert set(sa) == set(sb) and all(_same(sa[k], sb[k]) for k in sb), (sa, sb)
    assert 0.0 < rb["tol"] < float("inf")


_LOGS = {}


def _launch_logs():
    """the launch log (PYAPES_HIP_DEBUG) of the cases above in ONE child process, a marker per solve: one CG iteration of
    every prologue case, two Jacobi sweep pairs and two BiCGSTAB iterations of OTHER_METHOD_CASES, and the
    coefficient-field sweep.  (The log is limited per kernel instantiation; k_cg2d's pitched and
    plain forms share one budget, so the pitched case runs first.)"""
    if not _LOGS:
        import subprocess
        import sys
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
                "from test_gpu_fold import PROLOGUE_CASES, OTHER_METHOD_CASES, _prologue_solve, _cf_jacobi_solve\n"
                "def mark(s): sys.stderr.write('CASE ' + s + '\\n'); sys.stderr.flush()\n"
                "for name in PROLOGUE_CASES:\n"
                "    mark(name + ' cg'); _prologue_solve(name, 'cg', 1, -1.0, 0)\n"
                "for name, method in OTHER_METHOD_CASES:\n"
                "    mark(name + ' ' + method); _prologue_solve(name, method, 1, -1.0, 2)\n"
                "mark('cf_jacobi'); _cf_jacobi_solve(1, 1)\n" % (root, os.path.join(root, "oracle"), os.path.join(root, "tests")))
        p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                           env=dict(os.environ, PYAPES_HIP_DEBUG="1", PYAPES_HIP_RESIDENT="0"))
        assert p.returncode == 0, p.stderr[-2000:]
        _LOGS.update({seg.split("\n", 1)[0].strip(): seg for seg in p.stderr.split("CASE ")[1:]})
    return _LOGS


# (case, method): phases of the launch log that the solve must name -- E / J the Jacobi sweep forwards / backwards, G
# BiCGSTAB's s / t phase, I its v phase from a stored p
OTHER_METHOD_CASES = {("cg3d_vector_f64", "jacobi"): "EJ", ("cg3d_narrow_f64", "jacobi"): "EJ", ("cg2d_f64", "jacobi"): "EJ",
                      ("cg3d_vector_f64", "bicgstab"): "GI", ("cg3d_pitched_f64", "bicgstab"): "GI", ("cg2d_f64", "bicgstab"): "GI"}


def test_every_prologue_case_runs_the_kernel_it_names():
    """without this the comparison above could pass on the generic kernels or on another layout"""
    logs = _launch_logs()
    assert set(logs) == {name + " cg" for name in PROLOGUE_CASES} | {"%s %s" % k for k in OTHER_METHOD_CASES} | {"cf_jacobi"}
    for name, case in PROLOGUE_CASES.items():
        kernel, tag = case[5], case[6]
        for phase in "AB":
            assert "%s phase %s%s:" % (kernel, phase, tag) in logs[name + " cg"], (name, logs[name + " cg"][-1500:])
    for (name, method), phases in OTHER_METHOD_CASES.items():
        kernel, tag = PROLOGUE_CASES[name][5], PROLOGUE_CASES[name][6]
        for phase in phases:
            assert "%s phase %s%s:" % (kernel, phase, tag) in logs["%s %s" % (name, method)], (name, method, logs["%s %s" % (name, method)][-1500:])


def test_coefficient_field_sweep_keeps_six_blocks_per_cu():
    """its launch-log lines: both directions of the sweep, one tile, and chunks = 6 blocks / CU x the CUs -- the figure the
    partial sums of this instantiation have always been grouped by (the kernel itself would fit 7 since its prologue is
    the shared one)"""
    import re
    log = _launch_logs()["cf_jacobi"]
    for phase in "EJ":
        m = re.search(r"k_cg3d phase %s \(narrow\): tiles 1x1 chunks (\d+) \(CI ~\d+\) blocks (\d+), (\d+) blocks/CU x (\d+) CUs" % phase, log)
        assert m, log[-1500:]
        chunks, blocks, bpc, cus = (int(v) for v in m.groups())
        assert bpc == 6 and chunks == blocks == min(CF_JACOBI_N[0], 6 * cus), m.group(0)


def test_rhs_adjust_on_the_neumann_layers_only(monkeypatch):
    """The rhs adjustment touches the nodes one step inside a Neumann face; the kernel visits those layers
    (a node on two layers once) instead of the whole mesh (option rhs_full): same bits."""
    from pyapes_amd.hip import lib as L
    from pyapes_amd.hip.context import context_for
    rng = random.Random(99)
    seen = 0
    for case in range(60):
        nd = rng.choice([1, 2, 3])
        n = [rng.choice([3, 4, 5, 8, 17, 33]) for _ in range(nd)]
        bcs = []
        for a in range(nd):
            for _ in range(2):
                t = rng.choice(["dirichlet", "neumann", "neumann", "symmetry"])
                bcs.append((t, None if t == "symmetry" else round(rng.uniform(-1, 1), 3)))
        if not any(t == "neumann" for t, _ in bcs):
            continue
        dtype = rng.choice(["double", "single"])
        tdt = torch.float64 if dtype == "double" else torch.float32
        mesh = Mesh(Box([0.0] * nd, [1.0 + 0.1 * a for a in range(nd)]), None, list(n), "cuda", dtype)
        cfg = [{"bc_face": _faces()[i], "bc_type": t, "bc_val": v, "bc_val_opt": None} for i, (t, v) in enumerate(bcs)]
        var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
        ctx = context_for(mesh)
        ctx.bind_bcs(var(), var.bcs, 0)
        terms = [{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": 0.7}]
        if nd == 1:
            terms.append({"kind": L.OP_GRAD, "sign": 1.0, "coeff": 0.3})
        ctx.set_terms(terms)
        g = torch.Generator().manual_seed(case)
        rhs = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt).cuda()
        a, b = rhs.clone(), rhs.clone()
        ctx.set_option("rhs_full", 0)
        ctx.rhs_adjust(a[0])
        ctx.set_option("rhs_full", 1)
        ctx.rhs_adjust(b[0])
        ctx.set_option("rhs_full", 0)
        assert torch.equal(a, b), (case, n, bcs, dtype)
        assert not torch.equal(a, rhs) or all(v == 0 for t, v in bcs if t == "neumann")
        seen += 1
    assert seen >= 30
