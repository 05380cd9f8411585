"""-m gpu: the solvers, the explicit operators, A x and the BC fill on operands that are NOT 16-byte aligned.

Every tiled launcher picks its kernel from the addresses of its operands as well as from the mesh (cg3d_mode,
csrc/pa_cg3d_kernel.h; k_bicg_x's VV = 1 form; k_copy_guarded's scalar branch; solver_pitch), and the host layer hands a
caller's tensor through untouched, so a contiguous view one element into a larger allocation reaches all of those forks.
In CG that puts the PHASES OF ONE SOLVE ON DIFFERENT TILINGS: phase A streams ctx-owned arrays only (vector lanes), phase
B's operand list holds the caller's x (one cell per lane, NARROW; a tiled k_cg2d phase A beside a NARROW k_cg3d phase B
on a 2-D mesh; a tiled phase A beside the generic phase B on an axisymmetric one), and the partial rows one phase
leaves for the other's prologue are counted on another tile grid.

The library is driven through the context methods on views, the way linalg._run and Solver.set_eq drive it.  Every operand
lies inside an allocation with sentinel guards (helpers.offset_view): no access leaves live memory, and a store outside
the array shows up as a changed guard.  The criteria are the ones the suite already applies to these kernels
(test_gpu_fastpath.py, test_gpu_cg2d.py, test_gpu_pitched.py, test_gpu_tiled_ops.py, test_gpu_resident.py,
test_gpu_more_ops.py, test_gpu_fold.py); the yardsticks are the generic kernels, the same call on aligned operands and the
CPU oracle.  The module switches the resident solver off itself (part (f) switches it on)."""
import contextlib
import re
import warnings

import pytest
import torch

import march_gpu as G
import pyapes_oracle as O
from helpers import guards_intact, offset_view, rel_err
from pyapes_amd.geometry import Box, Cylinder
from pyapes_amd.hip import lib as L
from pyapes_amd.hip.context import context_for
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import div_kind
from pyapes_amd.solver.fdm import FDM
from pyapes_amd.solver.ops import Solver
from pyapes_amd.variables import Field

pytestmark = pytest.mark.gpu

D = lambda v=0.0: ("dirichlet", v)   # noqa: E731
N = lambda v=0.0: ("neumann", v)     # noqa: E731
SY = ("symmetry", None)
PE = ("periodic", None)

# name -> (n, dtype, lower, upper, coord).  The smallest meshes on which the forks still differ: partial j and k tiles and
# 2 (fp64) / 1 (fp32) vector k-tiles against 3 NARROW ones; the shortest row the vector layout accepts (2 vectors); a 2-D
# and an axisymmetric mesh for k_cg2d (option cg2d_mincells 0); odd rows for the PITCH layout.
MESHES = {
    "3d_f64": ([7, 18, 132], "double", [0.0, 0.0, 0.0], [1.0, 1.0, 0.5], "xyz"),
    "3d_f32": ([7, 18, 132], "single", [0.0, 0.0, 0.0], [1.0, 1.0, 0.5], "xyz"),
    "short_f64": ([5, 9, 4], "double", [0.0, 0.0, 0.0], [1.0, 1.0, 0.5], "xyz"),
    "short_f32": ([5, 9, 8], "single", [0.0, 0.0, 0.0], [1.0, 1.0, 0.5], "xyz"),
    "2d_f64": ([48, 132], "double", [0.0, 0.0], [1.0, 1.0], "xyz"),
    "2d_f32": ([48, 132], "single", [0.0, 0.0], [1.0, 1.0], "xyz"),
    "rz_f64": ([24, 32], "double", [0.0, 0.0], [1.0, 1.5], "rz"),
    "odd_f64": ([7, 18, 133], "double", [0.0, 0.0, 0.0], [1.0, 1.0, 0.5], "xyz"),
    # keep_old only: node counts that are no multiple of the 16-byte vector (16758 = 2 mod 4 in fp32, 8379 odd in fp64)
    "odd_f32": ([7, 18, 133], "single", [0.0, 0.0, 0.0], [1.0, 1.0, 0.5], "xyz"),
    "oddcount_f64": ([7, 9, 133], "double", [0.0, 0.0, 0.0], [1.0, 1.0, 0.5], "xyz"),
}
# the BC sets of test_gpu_fastpath.py ("dir": static, no fill per iteration; "mix": a fill per iteration; "per": shell
# terms, rhs without its mean; "zper"), their 2-D restrictions, and the set test_gpu_rz.py solves
BCS3 = {
    "dir": [D(0.0)] * 6,
    "mix": [D(0.0), N(0.5), D(0.3), N(0.0), D(1.0), N(-0.25)],
    "per": [PE] * 6,
    "zper": [D(0.5), N(0.1), SY, D(0.0), PE, PE],
}
BCS2 = {
    "dir": [D(0.0)] * 4,
    "mix": [D(0.0), N(0.5), D(1.0), N(-0.25)],
    "per": [PE] * 4,
    "zper": [D(0.5), N(0.1), PE, PE],     # the contiguous axis periodic
}
BCSRZ = {"mixrz": [N(0.0), D(1.0), D(0.3), N(0.5)]}
K = 6                 # max_it of CG / BiCGSTAB (CG executes max_it + 1 iterations, BiCGSTAB max_it)
K_JACOBI = 12         # max_it of Jacobi: 13 sweeps, an odd count, so the final iterate is copied back into the caller's x
SEED = 20240


def _bcs_of(mname):
    n, _, _, _, coord = MESHES[mname]
    return BCSRZ if coord == "rz" else (BCS3 if len(n) == 3 else BCS2)


def _offsets(mname):
    """misalignments in elements: 8 bytes in fp64; 4 and 8 bytes in fp32 (both off 16)"""
    return (1,) if MESHES[mname][1] == "double" else (1, 2)


def _f64(mname):
    return MESHES[mname][1] == "double"


_SETUP = {}


def _setup(mname, bc):
    """(mesh, ctx, field that owns the BC objects, oracle mesh, oracle BC config) -- one mesh and context per mesh name"""
    if (mname, bc) not in _SETUP:
        n, dtype, lo, hi, coord = MESHES[mname]
        if mname not in _SETUP:
            geo = Cylinder(lo, hi) if coord == "rz" else Box(lo, hi)
            mesh = Mesh(geo, None, list(n), "cuda", dtype)
            _SETUP[mname] = (mesh, context_for(mesh), O.OMesh(lo, hi, list(n), dtype, coord))
        mesh, ctx, om = _SETUP[mname]
        faces = O.FACES_RZ if coord == "rz" else O.FACES
        ocfg = [{"bc_face": faces[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(_bcs_of(mname)[bc])]
        var = Field("p", 1, mesh, {"domain": [dict(c, bc_val_opt=None) for c in ocfg], "obstacle": None})
        _SETUP[(mname, bc)] = (mesh, ctx, var, om, ocfg)
    return _SETUP[(mname, bc)]


def _options(ctx, fast=True, fold=True, pitch=True, resident=False):
    ctx.set_option("resident", resident)
    ctx.set_option("cg2d_mincells", 0)       # k_cg2d on the small 2-D / axisymmetric meshes (3-D meshes never take it)
    ctx.set_option("fastpath", fast)
    ctx.set_option("fold", fold)
    ctx.set_option("pitch", pitch)


@contextlib.contextmanager
def _reaching(ctx):
    """the device pointers the context hands to the C ABI while the block runs (every tensor goes through ctx._ptr; the
    coefficient tensor of a term is kept by set_terms)"""
    seen = []
    orig = ctx._ptr

    def spy(t):
        seen.append(0 if t is None else t.data_ptr())
        return orig(t)

    ctx._ptr = spy
    try:
        yield seen
    finally:
        del ctx._ptr


def _assert_reached(seen, view, misaligned, what):
    assert view.data_ptr() in seen, f"{what}: the view's pointer did not reach the call (a copy was made)"
    assert (view.data_ptr() % 16 != 0) == misaligned, (what, view.data_ptr() % 16)


def _tdt(mname):
    return torch.float64 if _f64(mname) else torch.float32


# ======================================================================================================================
#  (a) single launches, bit for bit
# ======================================================================================================================
U_SCALAR = 1.3
FILL = 3.25           # what an output holds before the call (both kernels under comparison write every node)

_INPUTS = {}


def _inputs(mname, bc):
    """CPU tensors of one (mesh, BC set), from a fixed seed: a BC-filled field, an unfilled one, a speed, a coefficient"""
    if (mname, bc) not in _INPUTS:
        mesh, ctx, var, om, ocfg = _setup(mname, bc)
        n, tdt = MESHES[mname][0], _tdt(mname)
        g = torch.Generator().manual_seed(SEED)
        raw = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        ut = (0.5 + torch.randn((1, *n), generator=g, dtype=torch.float64)).to(tdt)
        gamma = (1.0 + 0.2 * torch.rand((1, *n), generator=g, dtype=torch.float64)).to(tdt)
        x = raw.clone()
        O.bc_fill(x, O.make_bcs(om, ocfg))
        _INPUTS[(mname, bc)] = {"x": x, "raw": raw, "u": ut, "gamma": gamma}
    return _INPUTS[(mname, bc)]


# op -> (roles in call order, the role that is written)
def _op_table(mname, bc):
    nd = len(MESHES[mname][0])
    ops = {
        "lap": (("x", "out"), "out"),
        "grad": (("x", "gout"), "gout"),
        "aop_scalar": (("x", "out"), "out"),
        "aop_tensor": (("x", "gamma", "out"), "out"),
        "apply_bc": (("raw",), "raw"),
        "rhs_adjust": (("zero",), "zero"),
    }
    lims = ["upwind", "compat"] + (["none"] if bc == "per" else [])   # central Div refuses neumann / symmetry faces
    for lim in lims:
        ops[f"div_{lim}_s"] = (("x", "out"), "out")
        ops[f"div_{lim}_t"] = (("x", "u", "out"), "out")
    assert nd in (2, 3)
    return ops


def _source(mname, bc, role):
    inp = _inputs(mname, bc)
    n, tdt = MESHES[mname][0], _tdt(mname)
    if role in inp:
        return inp[role]
    if role == "out":
        return torch.full((1, *n), FILL, dtype=tdt)
    if role == "gout":
        return torch.full((len(n), *n), FILL, dtype=tdt)
    assert role == "zero"
    return torch.zeros((1, *n), dtype=tdt)


def _run_op(mname, bc, op, t, fast):
    """one launch of `op` on the tensors `t` (role -> (1, *n) device tensor); returns the pointers that reached the call"""
    mesh, ctx, var, om, ocfg = _setup(mname, bc)
    _options(ctx, fast=fast)
    kept = []
    with _reaching(ctx) as seen:
        if op == "rhs_adjust":     # Solver.set_eq / fdc._rhs_adjust: the bare term, the BC list bound for the rhs
            ctx.bind_bcs(t["zero"], var.bcs, 0, for_rhs=True)
            ctx.set_terms([{"kind": L.OP_LAPLACIAN}])
            ctx.rhs_adjust(t["zero"][0])
        elif op == "apply_bc":
            ctx.bind_bcs(t["raw"], var.bcs, 0)
            ctx.apply_bc_bound(t["raw"][0])
        else:
            ctx.bind_bcs(t["x"], var.bcs, 0)
            if op == "lap":
                ctx.laplacian(t["x"][0], False, out=t["out"][0])
            elif op == "grad":
                ctx.grad(t["x"][0], False, out=t["gout"])
            elif op == "aop_scalar":
                ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": 0.7}])
                ctx.aop(t["x"][0], out=t["out"][0])
            elif op == "aop_tensor":
                ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": 1.0, "coeff": t["gamma"]}])
                kept = [k.data_ptr() for k in ctx._keep["terms"][1]]
                ctx.aop(t["x"][0], out=t["out"][0])
            else:
                _, lim, speed = op.split("_")
                kind = div_kind("upwind" if lim == "compat" else lim, lim == "compat")
                ctx.div(kind, U_SCALAR if speed == "s" else t["u"], t["x"][0], out=t["out"][0])
    return seen + kept


_ORACLE_OPS = {}


def _oracle_op(mname, bc, op):
    """the oracle's statement of `op` where the suite holds it to a bit-exact criterion (tests/test_oracle_golden.py,
    test_gpu_parity_golden.py::test_ops_bit_exact, test_gpu_more_ops.py), else None"""
    key = (mname, bc, op)
    if key not in _ORACLE_OPS:
        mesh, ctx, var, om, ocfg = _setup(mname, bc)
        inp = _inputs(mname, bc)
        nd = len(MESHES[mname][0])
        bcs = O.make_bcs(om, ocfg)
        x = inp["x"].clone()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if op == "lap":
                r = O.apply_laplacian(O.laplacian_tables(x, om, bcs), x, nd)
            elif op == "grad":
                r = O.apply_grad(O.grad_tables(x, om, bcs), x, nd)[0]
            elif op == "aop_scalar":
                r = O.Aop(x, [O.OTerm("laplacian", O.laplacian_tables(x, om, bcs), 0.7, -1.0)], nd)
            elif op == "aop_tensor":
                r = O.Aop(x, [O.OTerm("laplacian", O.laplacian_tables(x, om, bcs), inp["gamma"].clone(), 1.0)], nd)
            elif op == "apply_bc":
                r = O.bc_fill(inp["raw"].clone(), bcs)
            elif op == "rhs_adjust":
                r = O.laplacian_rhs_adjust(torch.zeros_like(x), om, bcs)
            elif op.startswith("div_compat") or op.startswith("div_none"):
                u = U_SCALAR if op.endswith("_s") else inp["u"].clone()
                r = O.apply_div(O.div_tables(u, x, om, bcs, "upwind" if "compat" in op else "none"), x, nd)
            else:
                r = None   # the intended upwind form: the suite pins it bit for bit in 1-D only
        _ORACLE_OPS[key] = r
    return _ORACLE_OPS[key]


OP_MESHES = ["3d_f64", "3d_f32", "short_f64", "short_f32", "2d_f64", "rz_f64", "odd_f64"]


@pytest.mark.parametrize("mname,bc", [(m, b) for m in OP_MESHES for b in _bcs_of(m)], ids=lambda v: v)
def test_single_launches_bit_for_bit(mname, bc):
    """every operand role misaligned alone, then all at once: the tiled launch equals the generic kernels on the same
    views, the same call on aligned operands and the oracle, bit for bit; guards intact; inputs unchanged"""
    for op, (roles, written) in _op_table(mname, bc).items():
        src = {r: _source(mname, bc, r) for r in roles}
        al = {r: offset_view(src[r].cuda(), 0)[0] for r in roles}
        _run_op(mname, bc, op, al, True)
        aligned = al[written].clone()
        oracle = _oracle_op(mname, bc, op)
        if oracle is not None:
            assert torch.equal(aligned.cpu(), oracle), (op, "aligned vs oracle", float((aligned.cpu() - oracle).abs().max()))
        configs = [(r,) for r in roles] + ([tuple(roles)] if len(roles) > 1 else [])
        for mis in configs:
            for off in _offsets(mname):
                pairs = {r: offset_view(src[r].cuda(), off if r in mis else 0) for r in roles}
                t = {r: p[0] for r, p in pairs.items()}
                seen = _run_op(mname, bc, op, t, True)
                for r in roles:
                    _assert_reached(seen, t[r], r in mis, (op, mis, off, r))
                tiled = t[written].clone()
                for r in roles:
                    assert guards_intact(pairs[r][1], t[r]), (op, mis, off, r, "guard")
                    if r != written:
                        assert torch.equal(t[r].cpu(), src[r]), (op, mis, off, r, "input changed")
                t[written].copy_(src[written].cuda())
                _run_op(mname, bc, op, t, False)
                generic = t[written]
                what = (op, mis, off)
                assert torch.equal(tiled, generic), (what, "tiled vs generic", float((tiled - generic).abs().max()))
                assert torch.equal(tiled, aligned), (what, "misaligned vs aligned", float((tiled - aligned).abs().max()))
                if oracle is not None:
                    assert torch.equal(tiled.cpu(), oracle), (what, "vs oracle")
                for r in roles:
                    assert guards_intact(pairs[r][1], t[r]), (op, mis, off, r, "guard (generic)")


# ======================================================================================================================
#  (b) solves
# ======================================================================================================================
_RHS = {}


def _rhs(mname, bc):
    """(rhs0 on the CPU as the oracle takes it, the adjusted rhs on the device as Solver.set_eq leaves it) -- made once"""
    if (mname, bc) not in _RHS:
        mesh, ctx, var, om, ocfg = _setup(mname, bc)
        n, tdt = MESHES[mname][0], _tdt(mname)
        g = torch.Generator().manual_seed(SEED + 1)
        rhs0 = torch.randn((1, *n), generator=g, dtype=torch.float64)
        if bc == "per":
            rhs0 -= rhs0.mean()
        rhs0 = rhs0.to(tdt)
        adj, _ = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), 0)
        _options(ctx)
        ctx.bind_bcs(adj, var.bcs, 0, for_rhs=True)
        ctx.set_terms([{"kind": L.OP_LAPLACIAN}])
        ctx.rhs_adjust(adj[0])
        _RHS[(mname, bc)] = (rhs0, rhs0.cuda() + adj)
    return _RHS[(mname, bc)]


def _max_it(method):
    return K_JACOBI if method == "jacobi" else K


def _solve(mname, bc, method, x, rhs, max_it=None, x_old=None, coeff=0.7, tol=1e-30, **opts):
    """linalg._run on views: bind the list, set the term, keep_old, solve.  Returns (itr, tol, scalars, pointers)."""
    mesh, ctx, var, om, ocfg = _setup(mname, bc)
    _options(ctx, **opts)
    with _reaching(ctx) as seen:
        ctx.bind_bcs(x, var.bcs, 0)
        ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": coeff}])
        ctx.keep_old(None if x_old is None else x_old[0])
        try:
            rep = ctx.solve(method, x[0], rhs[0], tol, _max_it(method) if max_it is None else max_it, omega=0.9)
        finally:
            ctx.keep_old(None)
    return int(rep.itr), float(rep.tol), ctx.scalars(), seen


_ORACLE_SOLVE = {}


def _oracle_solve(mname, bc, method, max_it=None):
    key = (mname, bc, method, max_it)
    if key not in _ORACLE_SOLVE:
        mesh, ctx, var, om, ocfg = _setup(mname, bc)
        kw = {"omega": 0.9} if method == "jacobi" else {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _ORACLE_SOLVE[key] = O.solve_poisson(om, ocfg, _rhs(mname, bc)[0].clone(), method=method, tol=1e-30,
                                                 max_it=_max_it(method) if max_it is None else max_it, coeff=0.7,
                                                 sign=-1.0, **kw)[:2]
    return _ORACLE_SOLVE[key]


def _check_vs_oracle(mname, x, itr, tol, xo, ro, what):
    f64 = _f64(mname)
    e = rel_err(x.cpu(), xo)
    print(what, "vs oracle: rel_err %.3e itr %d/%d tol %.9e/%.9e" % (e, itr, ro["itr"], tol, ro["tol"]))
    assert itr == ro["itr"], (what, itr, ro["itr"])
    assert e <= (1e-10 if f64 else 1e-5), (what, e)
    assert abs(tol - ro["tol"]) <= (1e-6 if f64 else 1e-4) * abs(ro["tol"]), (what, tol, ro["tol"])


def _check_vs_other_grouping(mname, method, x, itr, sc, xa, itra, sca, what):
    """against the same solve on aligned operands: only the grouping of the global sums may differ"""
    f64 = _f64(mname)
    e = rel_err(x.cpu(), xa.cpu())
    print(what, "vs aligned: rel_err %.3e" % e, {k: (sc[k], sca[k]) for k in ("alpha", "beta", "omega", "tol")})
    assert itr == itra, (what, itr, itra)
    if method == "jacobi":    # no global sum feeds back into the iterate
        assert torch.equal(x, xa), (what, float((x - xa).abs().max()))
        return
    if method == "cg":
        assert e < (1e-12 if f64 else 2e-6), (what, e)
        keys, rt = ("alpha", "beta", "tol"), (1e-10 if f64 else 1e-4)
    else:
        assert e < (1e-11 if f64 else 5e-6), (what, e)
        keys, rt = ("alpha", "omega", "tol"), (1e-9 if f64 else 1e-3)
    for k in keys:
        assert abs(sc[k] - sca[k]) <= rt * abs(sca[k]), (what, k, sc[k], sca[k])


SOLVE_MESHES = ["3d_f64", "3d_f32", "short_f64", "short_f32", "2d_f64", "2d_f32", "rz_f64"]
ROLES = {"x": ("x",), "rhs": ("rhs",), "both": ("x", "rhs")}


@pytest.mark.parametrize("method", ["cg", "bicgstab", "jacobi"])
@pytest.mark.parametrize("mname,bc", [(m, b) for m in SOLVE_MESHES for b in _bcs_of(m)], ids=lambda v: v)
def test_solve_on_misaligned_operands(mname, bc, method):
    """x alone, rhs alone and both misaligned: against the oracle, the generic kernels on the same views and the same solve
    on aligned operands; guards around x intact, rhs unchanged"""
    f64 = _f64(mname)
    n, tdt = MESHES[mname][0], _tdt(mname)
    rhs_dev = _rhs(mname, bc)[1]
    xo, ro = _oracle_solve(mname, bc, method)
    xa, _ = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), 0)
    ra, _ = offset_view(rhs_dev, 0)
    itra, tola, sca, _ = _solve(mname, bc, method, xa, ra)
    _check_vs_oracle(mname, xa, itra, tola, xo, ro, (mname, bc, method, "aligned"))
    for role, mis in ROLES.items():
        for off in _offsets(mname):
            what = (mname, bc, method, role, off)
            x, xalloc = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), off if "x" in mis else 0)
            rhs, ralloc = offset_view(rhs_dev, off if "rhs" in mis else 0)
            itr, tol, sc, seen = _solve(mname, bc, method, x, rhs)
            _assert_reached(seen, x, "x" in mis, what + ("x",))
            _assert_reached(seen, rhs, "rhs" in mis, what + ("rhs",))
            assert guards_intact(xalloc, x) and guards_intact(ralloc, rhs), what
            assert torch.equal(rhs, rhs_dev), what + ("rhs changed",)
            xt = x.clone()
            _check_vs_oracle(mname, xt, itr, tol, xo, ro, what)
            _check_vs_other_grouping(mname, method, xt, itr, sc, xa, itra, sca, what)
            # the generic kernels on the same views
            x.zero_()
            itrg, tolg, scg, _ = _solve(mname, bc, method, x, rhs, fast=False)
            assert guards_intact(xalloc, x) and torch.equal(rhs, rhs_dev), what + ("generic",)
            e = rel_err(xt.cpu(), x.cpu())
            print(what, "vs generic: rel_err %.3e" % e)
            assert itr == itrg, (what, itr, itrg)
            if method == "jacobi":
                assert torch.equal(xt, x), (what, float((xt - x).abs().max()))
            assert e <= (1e-12 if f64 else 2e-5), (what, "vs generic", e)


def test_public_path_keeps_the_misaligned_storage():
    """Field.set_var_tensor(view), Solver.set_eq, Solver.solve(): the view's storage is what is solved in"""
    mname, bc = "3d_f64", "mix"
    mesh, ctx, var0, om, ocfg = _setup(mname, bc)
    n, tdt = MESHES[mname][0], _tdt(mname)
    _options(ctx)
    var = Field("p", 1, mesh, {"domain": [dict(c, bc_val_opt=None) for c in ocfg], "obstacle": None})
    x, xalloc = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), 1)
    rhs, ralloc = offset_view(_rhs(mname, bc)[0].cuda(), 1)
    var.set_var_tensor(x)
    assert var().data_ptr() == x.data_ptr() and x.data_ptr() % 16 != 0 and rhs.data_ptr() % 16 != 0
    s = Solver({"fdm": {"method": "cg", "tol": 1e-30, "max_it": K, "report": False}})
    s.set_eq(-FDM().laplacian(0.7, var) == rhs)
    assert s.rhs.data_ptr() == rhs.data_ptr()
    with _reaching(ctx) as seen, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = s.solve()
    assert var().data_ptr() == x.data_ptr()
    _assert_reached(seen, x, True, "public path x")
    _assert_reached(seen, rhs, True, "public path rhs")
    assert ctx.resident_used() == 0
    assert guards_intact(xalloc, x) and guards_intact(ralloc, rhs)
    assert torch.equal(rhs, _rhs(mname, bc)[1])          # set_eq adjusted the view in place
    xo, ro = _oracle_solve(mname, bc, "cg")
    _check_vs_oracle(mname, var(), rep["itr"], rep["tol"], xo, ro, "public path")


# ======================================================================================================================
#  (c) folded and unfolded scalar steps on mixed tilings
# ======================================================================================================================
def _stepwise(mname, bc, x, rhs, iters, fold):
    mesh, ctx, var, om, ocfg = _setup(mname, bc)
    _options(ctx, fold=fold)
    with _reaching(ctx) as seen:
        ctx.bind_bcs(x, var.bcs, 0)
        ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": 0.7}])
        ctx.cg_begin(x[0], rhs[0], 1e-30, 1000)
        try:
            ctx.cg_iterate(iters)
            rep = ctx.cg_end()
        except Exception:
            ctx.cg_abort()
            raise
    return rep, ctx.scalars(), seen


@pytest.mark.parametrize("mname,bc", [(m, b) for m in ("3d_f64", "3d_f32", "2d_f64", "rz_f64") for b in _bcs_of(m)],
                         ids=lambda v: v)
def test_folded_scalar_steps_on_mixed_tilings_same_bits(mname, bc):
    """cg_begin + cg_iterate(K) with x misaligned -- phase A and phase B on different tilings -- with the scalar steps in
    the next kernel's prologue (fold 1) and as kernels of their own (fold 0): the same bits in x and in the scalars"""
    n, tdt = MESHES[mname][0], _tdt(mname)
    rhs_dev = _rhs(mname, bc)[1]
    for off in _offsets(mname):
        out = {}
        for fold in (True, False):
            x, xalloc = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), off)
            rhs, _ = offset_view(rhs_dev, 0)
            rep, sc, seen = _stepwise(mname, bc, x, rhs, K, fold)
            _assert_reached(seen, x, True, (mname, bc, off, fold))
            assert guards_intact(xalloc, x)
            out[fold] = (x, int(rep.itr), float(rep.tol), sc)
        assert out[True][1] == out[False][1] == K
        assert torch.equal(out[True][0], out[False][0]), (off, float((out[True][0] - out[False][0]).abs().max()))
        assert out[True][2] == out[False][2]
        for k, v in out[True][3].items():
            w = out[False][3][k]
            assert v == w or (v != v and w != w), (off, k, v, w)
        # and it is the solve of (b): the one-shot loop on the same operands
        xs, _ = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), off)
        _solve(mname, bc, "cg", xs, offset_view(rhs_dev, 0)[0], max_it=K - 1)
        assert torch.equal(xs, out[True][0])


# ======================================================================================================================
#  (d) PITCH layout with an x that is sizeof(T)-aligned only
# ======================================================================================================================
@pytest.mark.parametrize("bc", ["dir", "mix"])
@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_pitched_layout_with_x_off_16_bytes(method, bc):
    """odd rows, x at 8 bytes: the ctx's arrays pitched, x touched cell by cell -- against the oracle and against pitch 0
    (the NARROW kernels) with the tolerances of test_gpu_pitched.py"""
    mname = "odd_f64"
    n, tdt = MESHES[mname][0], _tdt(mname)
    rhs_dev = _rhs(mname, bc)[1]
    k = K if method == "cg" else 5
    xo, ro = _oracle_solve(mname, bc, method, k)
    out = {}
    for pitch in (True, False):
        x, xalloc = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), 1)
        rhs, ralloc = offset_view(rhs_dev, 0)
        itr, tol, sc, seen = _solve(mname, bc, method, x, rhs, max_it=k, pitch=pitch)
        _assert_reached(seen, x, True, (method, bc, pitch))
        assert guards_intact(xalloc, x) and guards_intact(ralloc, rhs) and torch.equal(rhs, rhs_dev)
        out[pitch] = (x, itr, tol, sc)
    (xp, ip, tp, sp), (xn, inn, tn, sn) = out[True], out[False]
    _check_vs_oracle(mname, xp, ip, tp, xo, ro, ("pitched", method, bc))
    assert ip == inn
    e = rel_err(xp.cpu(), xn.cpu())
    print("pitched vs narrow", method, bc, "%.3e" % e)
    assert e < (1e-12 if method == "cg" else 1e-11), e
    for key in (("alpha", "beta", "tol") if method == "cg" else ("alpha", "omega", "tol")):
        assert abs(sp[key] - sn[key]) <= (1e-10 if method == "cg" else 1e-9) * abs(sn[key]), key


# ======================================================================================================================
#  (e) keep_old
# ======================================================================================================================
@pytest.mark.parametrize("method", ["cg", "bicgstab", "jacobi"])
@pytest.mark.parametrize("mname", ["odd_f32", "oddcount_f64"])
def test_keep_old_into_a_misaligned_buffer(mname, method):
    """x_old as a misaligned view (k_copy_guarded's scalar branch over the whole array) and as an aligned one whose length
    is no multiple of the vector (vector branch + tail): after K iterations it holds the iterate of the K - 1 run"""
    bc = "mix"
    n, tdt = MESHES[mname][0], _tdt(mname)
    assert (n[0] * n[1] * n[2]) % (2 if _f64(mname) else 4) != 0
    rhs_dev, _ = offset_view(_rhs(mname, bc)[1], 0)
    k = _max_it(method)
    prev, _ = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), 0)
    itp, _, _, _ = _solve(mname, bc, method, prev, rhs_dev, max_it=k - 1)
    for off in (0,) + _offsets(mname):
        x, xalloc = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), 0)
        old, oalloc = offset_view(torch.full((1, *n), FILL, dtype=tdt, device="cuda"), off)
        itr, _, _, seen = _solve(mname, bc, method, x, rhs_dev, max_it=k, x_old=old)
        _assert_reached(seen, old, off != 0, (mname, method, off))
        assert itr == itp + 1
        assert guards_intact(oalloc, old) and guards_intact(xalloc, x), (mname, method, off)
        assert torch.equal(old, prev), (mname, method, off, float((old - prev).abs().max()))
        assert not torch.equal(old, x)


# ======================================================================================================================
#  (f) resident solver
# ======================================================================================================================
@pytest.mark.parametrize("method,iters", [("cg", 8), ("bicgstab", 6)])
def test_resident_solver_on_misaligned_operands(method, iters):
    """test_gpu_resident.py::test_resident_vs_oracle with x and rhs misaligned"""
    n = [18, 14, 22]
    faces = [D(0.4), N(0.25), SY, D(-0.3), N(0.0), D(1.0)]
    ocfg = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(faces)]
    om = O.OMesh([0.0, 0.0, 0.0], [1.0, 1.1, 1.2], n, "double", "xyz")
    g = torch.Generator().manual_seed(21)
    rhs0 = torch.randn((1, *n), generator=g, dtype=torch.float64)
    x0 = torch.randn((1, *n), generator=g, dtype=torch.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xo, ro = O.solve_poisson(om, ocfg, rhs0.clone(), x0=x0.clone(), method=method, tol=-1.0, max_it=iters - 1,
                                 coeff=0.8, sign=-1.0)[:2]
    mesh = Mesh(Box([0.0, 0.0, 0.0], [1.0, 1.1, 1.2]), None, n, "cuda", "double")
    ctx = context_for(mesh)
    ctx.set_option("resident", True)
    var = Field("p", 1, mesh, {"domain": [dict(c, bc_val_opt=None) for c in ocfg], "obstacle": None})
    x, xalloc = offset_view(x0.cuda(), 1)
    adj, _ = offset_view(torch.zeros((1, *n), dtype=torch.float64, device="cuda"), 0)
    ctx.bind_bcs(x, var.bcs, 0, for_rhs=True)
    ctx.set_terms([{"kind": L.OP_LAPLACIAN}])
    ctx.rhs_adjust(adj[0])
    rhs, ralloc = offset_view(rhs0.cuda() + adj, 1)
    keep = rhs.clone()
    with _reaching(ctx) as seen:
        ctx.bind_bcs(x, var.bcs, 0)
        ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": 0.8}])
        ctx.keep_old(None)
        rep = ctx.solve(method, x[0], rhs[0], -1.0, iters - 1)
    _assert_reached(seen, x, True, "resident x")
    _assert_reached(seen, rhs, True, "resident rhs")
    assert ctx.resident_used() > 0
    assert guards_intact(xalloc, x) and guards_intact(ralloc, rhs) and torch.equal(rhs, keep)
    assert rep.itr == ro["itr"]
    assert float((x.cpu() - xo).abs().max()) <= (1e-9 if method == "bicgstab" else 1e-11) * float(xo.abs().max())
    assert rep.tol == pytest.approx(ro["tol"], rel=1e-9)


# ======================================================================================================================
#  (g) the forks are really taken
# ======================================================================================================================
FORK_CASES = [("3d", "3d_f64", "mix"), ("2d", "2d_f64", "mix"), ("rz", "rz_f64", "mixrz"), ("pitch", "odd_f64", "mix")]


def fork_case(mname, bc):
    """two CG iterations with x one element off alignment (the child process of the test below calls this)"""
    n, tdt = MESHES[mname][0], _tdt(mname)
    x, _ = offset_view(torch.zeros((1, *n), dtype=tdt, device="cuda"), 1)
    assert x.data_ptr() % 16 != 0
    _stepwise(mname, bc, x, offset_view(_rhs(mname, bc)[1], 0)[0], 2, True)


def test_the_phases_of_one_solve_run_on_different_tilings():
    """the launch log (PYAPES_HIP_DEBUG) of CG with x misaligned, one child process, a marker per case (the log is limited
    per kernel instantiation)"""
    code = ("import torch\nimport test_gpu_unaligned as U\n"
            "for name, mname, bc in U.FORK_CASES:\n"
            "    U._rhs(mname, bc)\n"
            "    torch.cuda.synchronize(); sys.stderr.write('CASE %s\\n' % name); sys.stderr.flush()\n"
            "    U.fork_case(mname, bc)\n"
            "    torch.cuda.synchronize(); sys.stderr.flush()\n")
    seen = G.case_log(G.child(code), lambda ln: re.search(r"k_cg[23]d phase [AB]\b", ln) is not None)

    def lines(case, kernel, phase):
        return [ln for ln in seen[case] if f"{kernel} phase {phase}" in ln]

    def grid(ln):
        return re.search(r"tiles (\d+)x(\d+)", ln).groups()

    # 3-D: the vector phase A, the NARROW phase B, on different tile grids
    a, b = lines("3d", "k_cg3d", "A"), lines("3d", "k_cg3d", "B")
    assert a and b and not lines("3d", "k_cg2d", "A") and not lines("3d", "k_cg2d", "B"), seen["3d"]
    assert all("(narrow)" not in ln and "(pitched)" not in ln for ln in a), a
    assert all("(narrow)" in ln for ln in b), b
    assert grid(a[0]) != grid(b[0]), (a[0], b[0])
    # 2-D: k_cg2d's phase A beside the one-plane NARROW k_cg3d phase B
    assert lines("2d", "k_cg2d", "A") and not lines("2d", "k_cg3d", "A") and not lines("2d", "k_cg2d", "B"), seen["2d"]
    b = lines("2d", "k_cg3d", "B")
    assert b and all("(narrow)" in ln for ln in b), seen["2d"]
    # axisymmetric: the tiled phase A, no tiled phase B at all (the generic k_cg_b runs)
    assert lines("rz", "k_cg2d", "A") and not lines("rz", "k_cg3d", "A"), seen["rz"]
    assert not lines("rz", "k_cg2d", "B") and not lines("rz", "k_cg3d", "B"), seen["rz"]
    # odd rows: both phases pitched, whatever the alignment of x
    a, b = lines("pitch", "k_cg3d", "A"), lines("pitch", "k_cg3d", "B")
    assert a and b and all("(pitched)" in ln for ln in a + b), seen["pitch"]
