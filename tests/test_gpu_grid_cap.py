"""-m gpu: every kernel on meshes LARGER THAN ONE PASS OF ITS GRID (tests/grid_cap_cases.py states the meshes and the caps;
tests/test_grid_cap_host.py proves the properties from arithmetic).

1. the flat (grid-stride) kernels, option "fastpath" 0, on meshes of two and three passes, against the CPU oracle bit for bit;
2. the generic solver loops on the same meshes against the oracle at the bounds of tests/test_gpu_fuzz.py, folded and
   unfolded scalar steps and the BC-fill paths bit for bit among themselves;
3. tiled launches of more than PA_MAX_GRID blocks (one plane of more than 2048 tiles), where the drivers leave the folded
   prologue: against the oracle, the generic kernels and the unfolded sequence, and the launch log for the block counts.

Every test collects what differs and asserts once, with the figures; each counts the cases it ran."""
import re
import sys
import warnings

import pytest
import torch

import grid_cap_cases as C
import march_gpu as G
import march_ref as R
import pyapes_oracle as O
from helpers import bit_equal, rel_err
from pyapes_amd.hip.context import context_for
from pyapes_amd.solver.fdc import FDC, hessian, jacobian
from pyapes_amd.solver.fdm import FDM
from pyapes_amd.solver.ops import Solver
from pyapes_amd.variables import Field

pytestmark = pytest.mark.gpu


def _quiet(fn):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn()


def _mesh(mid, dtype, **options):
    """the mesh on the GPU with the launch-per-phase loops and ``options`` set on its context"""
    mesh = C.mesh_factory(mid, dtype)()
    ctx = context_for(mesh)
    ctx.set_option("resident", False)
    for k, v in options.items():
        ctx.set_option(k, v)
    return mesh, ctx


def _differs(got, want):
    """None when equal in every bit (a NaN equals a NaN), else the figures"""
    got, want = torch.as_tensor(got).cpu(), torch.as_tensor(want).cpu()
    if got.shape != want.shape or got.dtype != want.dtype:
        return ("kind", tuple(got.shape), tuple(want.shape), got.dtype, want.dtype)
    bad = (got != want) & ~(torch.isnan(got) & torch.isnan(want))
    if not bool(bad.any()):
        return None
    where = bad.flatten().nonzero().flatten()
    return (int(bad.sum()), "of", want.numel(), "flat indices", int(where[0]), "..", int(where[-1]),
            "largest difference", float((got.double() - want.double())[bad].abs().max()))


def _told(bad):
    return "%d differ: %s" % (len(bad), " | ".join(repr(b) for b in bad[:8]))


# =============================================================================================================================
#  1. the flat kernels beyond one pass
# =============================================================================================================================
STENCIL = [("one_and_a_bit", "double", "mixv"), ("one_and_a_bit", "single", "per"), ("three_trips", "single", "mix"),
           ("three_trips", "double", "dir"), ("line", "double", "mix"), ("line", "single", "per"), ("plane", "double", "xper"),
           ("plane", "single", "mixv"), ("rz_plane", "double", "rz"), ("rz_plane_off", "single", "rz")]


@pytest.mark.parametrize("mid,dtype,bcname", STENCIL, ids=["-".join(p) for p in STENCIL])
def test_stencil_operators_beyond_one_pass(mid, dtype, bcname):
    """k_aop, k_grad, k_edge and k_rhs_adjust through FDC.laplacian / grad / div (edge False and True; central, intended and
    literal upwind; a number and a tensor as the speed), their rhs_adj, and Aop / the adjusted right-hand side of a two-term
    equation: the oracle's bits at every node"""
    mesh, ctx = _mesh(mid, dtype, fastpath=0)
    om = C.omesh(mid, dtype)
    nd = om.dim
    dev_cfg, ocfg = C.bc_lists(mid, dtype, bcname, seed=3)
    obcs = O.make_bcs(om, ocfg)
    x = O.bc_fill(C.rand(mid, dtype, 1), obcs)
    ut = C.rand(mid, dtype, 2, scale=0.8)
    var = Field("p", 1, mesh, {"domain": dev_cfg, "obstacle": None})
    var.set_var_tensor(x.cuda())
    central = not any(t in ("neumann", "symmetry") for t, _ in C.faces_of(mid, bcname))   # (refused on such faces)
    rz = om.coord == "rz"
    bad, ran = [], 0

    def check(name, got, want):
        nonlocal ran
        ran += 1
        d = _differs(got, want)
        if d is not None:
            bad.append((name, d))

    def run():
        lap_o = O.apply_laplacian(O.laplacian_tables(x, om, obcs), x, nd)
        fdc = FDC({"laplacian": {"edge": False}})
        check("laplacian", fdc.laplacian(var), lap_o)
        check("laplacian rhs_adj", fdc.laplacian.rhs_adj, O.laplacian_rhs_adjust(x, om, obcs))
        O.edge_laplacian(lap_o, x, om)
        check("laplacian edge", FDC({"laplacian": {"edge": True}}).laplacian(var), lap_o)
        gr_o = O.apply_grad(O.grad_tables(x, om, obcs), x, nd)
        fdc = FDC({"grad": {"edge": False}})
        check("grad", fdc.grad(var), gr_o)
        check("grad rhs_adj", fdc.grad.rhs_adj, O.grad_rhs_adjust(x, om, obcs))
        O.edge_grad(gr_o, x, om)
        check("grad edge", FDC({"grad": {"edge": True}}).grad(var), gr_o)
        for tag, u_d, u_c in (("float", 0.7, 0.7), ("tensor", ut.cuda(), ut)):
            for lim in (["none"] if central else []) + ["upwind"]:
                fdc = FDC({"div": {"limiter": lim, "edge": False, "compat": True}})
                check(f"div {lim} compat {tag}", fdc.div(u_d, var), O.apply_div(O.div_tables(u_c, x, om, obcs, lim), x, nd))
                check(f"div {lim} compat {tag} rhs_adj", fdc.div.rhs_adj, O.div_rhs_adjust(u_c, x, om, obcs, lim))
            if not rz:    # the intended upwind form: the oracle's statement, the kernel's operation order (k_aop, kind 4)
                fdc = FDC({"div": {"limiter": "upwind", "edge": False}})
                check(f"div upwind {tag}", fdc.div(u_d, var), O.div_upwind_intended(u_c, x, om))
        if not rz:
            # a two-term equation, set but not solved: div(u, p) - 0.05 lap(p) with the literal upwind form and a tensor speed
            rhs0 = C.rand(mid, dtype, 4)
            rhs_d = rhs0.cuda()
            s = Solver({"fdm": {"method": "bicgstab", "tol": -1.0, "max_it": 1, "report": False}})
            fdm = FDM({"div": {"limiter": "upwind", "edge": False, "compat": True}})
            u_d = ut.cuda()
            s.set_eq(fdm.div(u_d, var) - fdm.laplacian(0.05, var) == rhs_d)
            spec = [{"kind": "div", "sign": 1.0, "u": ut, "limiter": "upwind"}, {"kind": "laplacian", "sign": -1.0, "coeff": 0.05}]
            terms, adjs = O.equation_terms(om, obcs, spec, x)
            check("two-term Aop", s.Aop(var), O.Aop(x, terms, nd))
            want = rhs0.clone()
            for a in adjs:
                want += a
            check("two-term rhs", rhs_d, want)

    _quiet(run)
    assert ran == {(True, False): 18, (False, False): 14, (False, True): 10}[(central, rz)], ran
    assert not bad, _told(bad)


BC_FILLS = [("one_and_a_bit", "double", "mixv"), ("three_trips", "single", "xper"), ("line", "double", "mix"),
            ("plane", "single", "dn"), ("rz_plane", "double", "rz"), ("big_shell", "double", "mix"), ("big_shell", "single", "per")]


@pytest.mark.parametrize("mid,dtype,bcname", BC_FILLS, ids=["-".join(p) for p in BC_FILLS])
def test_bc_fill_paths_beyond_one_pass(mid, dtype, bcname):
    """Field.apply_bcs on the default path of the mesh's shell size and on the forced ones (bc_path 1: pair kernels, 3: one
    launch per face, 4: the closed form): the oracle's bc_fill in every bit.  big_shell's shell takes two passes."""
    om = C.omesh(mid, dtype)
    raw = C.rand(mid, dtype, 6)
    bad, ran = [], 0
    for path in (None, 1, 3, 4):
        mesh, ctx = _mesh(mid, dtype, fastpath=0, **({} if path is None else {"bc_path": path}))
        dev_cfg, ocfg = C.bc_lists(mid, dtype, bcname, seed=5)
        if path is None:
            want = O.bc_fill(raw.clone(), O.make_bcs(om, ocfg))
            assert not torch.equal(want, raw)
        f = Field("q", 1, mesh, {"domain": dev_cfg, "obstacle": None})
        f.set_var_tensor(raw.cuda())
        f.apply_bcs()
        ran += 1
        d = _differs(f(), want)
        if d is not None:
            bad.append((path, d))
    assert ran == 4
    assert not bad, _told(bad)


GENERAL = [("one_and_a_bit", "single"), ("three_trips", "double"), ("line", "double"), ("plane", "double"), ("rz_plane", "double"),
           ("rz_plane_off", "single")]


@pytest.mark.parametrize("mid,dtype", GENERAL, ids=["-".join(p) for p in GENERAL])
def test_general_div_flux_and_rfp_beyond_one_pass(mid, dtype):
    """k_div_general (Jac advection; a vector target with a number, a tensor and a Field as advection; edge or not; central
    and the literal upwind form), k_diff_flux, jacobian / hessian (k_grad + k_edge) and, on the cylinders, k_rfp_friction /
    k_rfp_diffusion, as tests/test_gpu_fuzz.py::test_seeded_fuzz_explicit_operators compares them: the oracle's bits.  And
    the INTENDED upwind form of k_div_general (no test at any size had it), with its u phi / r term on the cylinders, against
    grid_cap_cases.div_general_upwind."""
    from pyapes_amd.solver.rfp import RFP
    mesh, ctx = _mesh(mid, dtype, fastpath=0)
    om = C.omesh(mid, dtype)
    nd, L = om.dim, om.letters
    rz = om.coord == "rz"
    phi, H, Gf = C.rand(mid, dtype, 31), C.rand(mid, dtype, 32), C.rand(mid, dtype, 33)
    ut = C.rand(mid, dtype, 34, lead=nd)
    mk = lambda name, t: Field(name, t.shape[0], mesh, {"domain": None, "obstacle": None}).set_var_tensor(t.cuda().clone())   # noqa: E731
    fphi, fH, fG = mk("phi", phi), mk("H", H), mk("G", Gf)
    bad, ran = [], 0

    def check(name, got, want):
        nonlocal ran
        ran += 1
        d = _differs(got, want)
        if d is not None:
            bad.append((name, d))

    def run():
        jac, hess = jacobian(fH), hessian(fG)
        jo, ho = O.jacobian(H[0], om), O.hessian(Gf[0], om)
        for a in range(nd):
            check("jacobian " + L[a], jac[L[a]], jo[L[a]])
            for b in range(a, nd):
                check("hessian " + L[a] + L[b], hess[L[a] + L[b]], ho[L[a] + L[b]])
        flux = FDC().diffFlux(hess, fphi)
        fo = O.diff_flux(ho, phi[0], om)
        check("diffFlux", flux(), fo)
        fu = mk("u", ut)
        for lim in ("none", "upwind"):
            for edge in (True, False):
                fdc = FDC({"div": {"limiter": lim, "edge": edge, "compat": True}})
                tag = f"{lim} edge={edge}"
                check("div jac " + tag, fdc.div(jac, fphi), O.apply_div(O.div_tables(jo, phi, om, [], lim), phi, nd, (om, jo) if edge else None))
                want = O.apply_div(O.div_tables(ut, fo, om, [], lim), fo, nd, (om, ut) if edge else None)
                check("div vector tensor " + tag, fdc.div(ut.cuda(), flux), want)
                check("div vector Field " + tag, fdc.div(fu, flux), want)
                check("div vector float " + tag, fdc.div(0.7, flux),
                      O.apply_div(O.div_tables(0.7, fo, om, [], lim), fo, nd, (om, 0.7) if edge else None))
        fdc = FDC({"div": {"limiter": "upwind", "edge": False}})
        if nd > 1:    # (a scalar target, edge False, a number or a tensor is the solver's operator k_aop: part of the stencil test)
            check("div intended vector tensor", fdc.div(ut.cuda(), flux), C.div_general_upwind(ut, fo, om))
            check("div intended vector Field", fdc.div(fu, flux), C.div_general_upwind(ut, fo, om))
            check("div intended vector float", fdc.div(-0.7, flux), C.div_general_upwind(-0.7, fo, om))
        check("div intended jac", fdc.div(jac, fphi), C.div_general_upwind(jo[L[0]].unsqueeze(0), phi, om))
        if rz:
            rfp = RFP()
            want = O.rfp_friction(jo, phi[0], om)
            check("friction", rfp.friction(jac, fphi).reshape(want.shape), want)
            want = O.rfp_diffusion(ho, phi[0], om)
            check("diffusion", rfp.diffusion(hess, fphi).reshape(want.shape), want)

    _quiet(run)
    base = nd + nd * (nd + 1) // 2 + 1 + 16
    assert ran == base + (4 if nd > 1 else 1) + (2 if rz else 0), ran
    assert not bad, _told(bad)


@pytest.mark.parametrize("dtype", ["double", "single"])
def test_limiters_beyond_one_pass(dtype):
    """k_limiter on 600 001 entries: +-0, +-inf, NaN, denormals and equal magnitudes of opposite sign, at the start, across
    the end of the first pass and at the end; the oracle's minmod / mc_limiter (rfp.py:262-286: a NaN operand gives 0)"""
    from pyapes_amd.solver.rfp import mc_limiter, minmod
    a, b = C.limiter_operands(dtype)
    bad, ran = [], 0
    for name, fn, want in (("minmod", minmod, O.minmod(a, b)), ("mc", mc_limiter, O.mc_limiter(a, b))):
        got = fn(a.cuda(), b.cuda()).cpu()
        ran += 1
        d = _differs(got, want)
        if d is not None:
            bad.append((name, d))
    assert ran == 2
    assert not bad, _told(bad)


# limiter -> the meshes (extents, dtype, BC set of march_gpu.BCS) its generic Euler kernel runs on: one with a partial second
# pass, and three_trips or line
EULER = [("upwind", "one_and_a_bit", "double", "mix"), ("upwind", "three_trips", "single", "xper"),
         ("none", "one_and_a_bit", "single", "dir"), ("none", "line", "double", "dir"),
         ("quick", "one_and_a_bit", "double", "mix"), ("quick", "line", "single", "dir"),
         ("minmod", "plane", "double", "xper"), ("minmod", "three_trips", "single", "mix"),
         ("mc", "one_and_a_bit", "single", "mix"), ("mc", "line", "double", "mix"), ("compat", "plane", "single", "mix")]


@pytest.mark.parametrize("limiter,mid,dtype,bcname", EULER, ids=["-".join(p) for p in EULER])
def test_generic_euler_step_and_stage_beyond_one_pass(limiter, mid, dtype, bcname):
    """k_euler (fastpath 0): one Euler step and one fused Runge-Kutta stage with a scalar speed of each sign and a speed
    field, and with source= (a field, on the step and the stage): tests/march_ref.py bit for bit"""
    n = C.MESHES[mid][0]
    mesh, bc, om, obcs, phis, phi0, ufield, src, nu, dt = G.setup(n, dtype, bcname, 1)
    ctx = context_for(mesh)
    ctx.set_option("resident", False)
    ctx.set_option("fastpath", 0)
    f = G.fresh_field(mesh, bc, phis)
    ctx.bind_bcs(f(), f.bcs, 0)
    c0, c1 = 0.75, 0.25
    phis_d, phi0_d = phis.cuda(), phi0.cuda()
    bad, ran = [], 0
    for tag, u, S in (("pos", 1.3, None), ("neg", -0.8, None), ("field", ufield, None), ("field+source", ufield, src)):
        u_d = u.cuda() if isinstance(u, torch.Tensor) else u
        S_d = None if S is None else S.cuda()[0]
        e = _quiet(lambda: R.euler_step(phis.clone(), u, nu, dt, om, obcs, limiter, *(() if S is None else (S,))))
        stage = (c0 * phi0) + (c1 * e)
        O.bc_fill(stage, obcs)
        out = torch.full_like(phis_d, float("nan"))
        ctx.euler_step(phis_d[0], out[0], G.kind(limiter), u_d, nu, dt, source=S_d)
        d = _differs(out, e)
        if d is not None:
            bad.append((tag, "step", d))
        out = torch.full_like(phis_d, float("nan"))
        ctx.rk_stage(phis_d[0], phi0_d[0], out[0], c0, c1, G.kind(limiter), u_d, nu, dt, source=S_d)
        d = _differs(out, stage)
        if d is not None:
            bad.append((tag, "stage", d))
        ran += 2
        assert not torch.equal(e, phis) and bool(torch.isfinite(e).all())
    assert ran == 8
    assert bit_equal(phis_d, phis) and bit_equal(phi0_d, phi0)
    assert not bad, _told(bad)


def test_momentum_step_beyond_one_pass():
    """one momentum_step (order 3, upwind; a vector field advecting itself) on the plane: march_ref.momentum bit for bit"""
    from pyapes_amd.solver.march import momentum_step
    from pyapes_amd.variables.bcs import mixed_bcs
    mesh, ctx = _mesh("plane", "double", fastpath=0)
    om = C.omesh("plane", "double")
    vals, types = G.MIXED[0][:4], G.MIXED[1][:4]          # one type per face, one value per component
    per_comp = [[None if v is None else v + 0.375 * c - 0.125 * f * c for f, v in enumerate(vals)] for c in range(2)]
    bc_v = {"domain": mixed_bcs([None if vals[f] is None else [per_comp[c][f] for c in range(2)] for f in range(4)], list(types)),
            "obstacle": None}
    obcs_v = [O.make_bcs(om, O.mixed_cfg(per_comp[c], types, O.FACES[:4])) for c in range(2)]
    dx = min(float(d) for d in mesh.dx_list)
    nu = 1e-3
    dt = 0.2 * min(dx * dx / (4 * nu), dx / 1.3)
    V = 0.5 * C.rand("plane", "double", 5, lead=2)
    for c in range(2):
        O.bc_fill(V[c:c + 1], obcs_v[c])
    f = Field("U", 2, mesh, bc_v)
    f.set_var_tensor(V.cuda())
    momentum_step(f, nu, dt, {"div": {"limiter": "upwind"}}, order=3)
    want = R.momentum.march(V, nu, dt, 1, om, obcs_v, "upwind", 3)
    assert _differs(f(), want) is None, _differs(f(), want)
    assert not torch.equal(want, V)


# =============================================================================================================================
#  2. and 3.: the solver loops
# =============================================================================================================================
def _bounds(method, dtype):
    """(iterate against the oracle, tiled against generic, scalars): tests/test_gpu_fuzz.py, tests/test_gpu_cg2d.py"""
    f64 = dtype == "double"
    if method == "bicgstab":
        return (1e-9 if f64 else 5e-5), (1e-10 if f64 else 5e-5), (1e-9 if f64 else 1e-3)
    return (1e-10 if f64 else 2e-5), (1e-12 if f64 else 1e-5), (1e-10 if f64 else 1e-4)


def _solve(case, save_old=False, **options):
    """Solver.set_eq + solve of a solver case from a zero start -> (x, report, ctx.scalars(), VARo or None), on the CPU"""
    mid, dtype, bc, method, iters = case
    mesh, ctx = _mesh(mid, dtype, **options)
    if bc == "poisson_rz":
        from pyapes_amd.testing.poisson import poisson_rz_bcs
        dev_cfg = poisson_rz_bcs()
    else:
        dev_cfg, _ = C.solve_cfgs(case)
    var = Field("p", 1, mesh, {"domain": dev_cfg, "obstacle": None})
    rhs, coeff, sign = C.solve_inputs(case)
    cfg = {"method": method, "tol": -1.0, "max_it": C.max_it_of(method, iters), "report": False, **C.solve_kw(method)}
    if save_old:
        cfg["save_old"] = True
    s = Solver({"fdm": cfg})
    lap = FDM().laplacian(coeff, var)
    s.set_eq((lap if sign > 0 else -lap) == rhs.cuda())
    rep = _quiet(s.solve)
    return var().cpu(), rep, ctx.scalars(), (var.VARo.cpu() if save_old else None)


def _same(a, b):
    return a == b or (a != a and b != b)


def _same_run(a, b):
    """what differs between two runs that must agree in every bit: iterate, itr, tol and every scalar"""
    out = []
    if not torch.equal(a[0], b[0]):
        out.append(("x", float((a[0] - b[0]).abs().max())))
    if a[1]["itr"] != b[1]["itr"] or not _same(a[1]["tol"], b[1]["tol"]):
        out.append(("report", a[1]["itr"], b[1]["itr"], a[1]["tol"], b[1]["tol"]))
    if set(a[2]) != set(b[2]):
        out.append(("scalar keys",))
    out += [(k, a[2][k], b[2][k]) for k in b[2] if k in a[2] and not _same(a[2][k], b[2][k])]
    return out


def _against_oracle(case, run, what, bad):
    mid, dtype, bc, method, iters = case
    xo, ro = C.oracle_solution(case)
    x_tol, _, s_tol = _bounds(method, dtype)
    err = rel_err(run[0], xo)
    dtol = abs(run[1]["tol"] - ro["tol"]) / abs(ro["tol"])
    print(f"{'-'.join(map(str, case))} {what}: itr {run[1]['itr']} (oracle {ro['itr']}) rel err {err:.3e} (bound {x_tol:g}) "
          f"tol {run[1]['tol']:.9e} (oracle {ro['tol']:.9e}, rel {dtol:.2e}, bound {s_tol:g})")
    if not (run[1]["itr"] == ro["itr"] == iters):
        bad.append((what, "itr", run[1]["itr"], ro["itr"]))
    if not err <= x_tol:
        bad.append((what, "iterate vs oracle", err, x_tol))
    if not dtol <= s_tol:
        bad.append((what, "tol vs oracle", run[1]["tol"], ro["tol"], dtol, s_tol))


SCALAR_KEYS = {"cg": ("alpha", "beta", "tol"), "bicgstab": ("alpha", "omega", "tol"), "jacobi": ("tol",)}


def _against_tiled(case, generic, tiled, tag, bad):
    """a generic run against a tiled one (fastpath 1) at the suite's tiled-versus-generic bounds: the iterate (Jacobi: bit for
    bit), the iteration count, and the scalars of the method at the relative bounds of tests/test_gpu_cg2d.py"""
    mid, dtype, bc, method, iters = case
    _, g_tol, s_tol = _bounds(method, dtype)
    err = rel_err(tiled[0], generic[0])
    print(f"{'-'.join(map(str, case))} {tag} vs generic: {err:.3e} (bound {g_tol:g})")
    if tiled[1]["itr"] != generic[1]["itr"]:
        bad.append((tag, "itr vs generic", tiled[1]["itr"], generic[1]["itr"]))
    if method == "jacobi":
        if not torch.equal(tiled[0], generic[0]):
            bad.append((tag, "Jacobi iterate vs generic: bits", err))
    elif not err <= g_tol:
        bad.append((tag, "iterate vs generic", err, g_tol))
    for key in SCALAR_KEYS[method]:
        if not abs(tiled[2][key] - generic[2][key]) <= s_tol * abs(generic[2][key]):
            bad.append((tag, "scalar vs generic", key, tiled[2][key], generic[2][key]))


@pytest.mark.parametrize("case", C.GENERIC_SOLVES, ids=lambda c: "-".join(map(str, c)))
def test_generic_solver_loops_beyond_one_pass(case):
    """CG, BiCGSTAB (3 iterations) and Jacobi (2 and 3 sweeps) on the generic kernels -- the phase kernels and their rows of
    per-block partial sums, the first-residual kernels, k_copy -- on two passes: the oracle's iteration count, iterate and
    tol; the folded scalar steps (fold 1) give the bits of the unfolded sequence.  The oracle reports no alpha, beta or
    omega: those are held, with tol, to the tiled kernels' run of the same case (fastpath 1, another grouping of every sum) at
    the relative bounds of tests/test_gpu_cg2d.py.  A 1-D mesh has no tiled kernels: on `line` the scalars have no
    independent check beyond the iterate and tol they produce."""
    mid, dtype, bc, method, iters = case
    bad = []
    folded = _solve(case, fastpath=0, fold=1)
    plain = _solve(case, fastpath=0, fold=0)
    _against_oracle(case, folded, "fold 1", bad)
    _against_oracle(case, plain, "fold 0", bad)
    bad += [("fold 1 vs fold 0", d) for d in _same_run(folded, plain)]
    if len(C.MESHES[mid][0]) > 1:
        _against_tiled(case, folded, _solve(case, fastpath=1, fold=1), "tiled", bad)
    assert not bad, _told(bad)


# the BC paths whose stop-test sum is grouped by the pair kernels (per axis), by BC set: bc_path 1 where the faces can be paired,
# and the default where the pair kernels are the default (a periodic axis, more than 150 k shell nodes)
PAIR_PATHS = {"mix": {1}, "xper": {None, 1}, "mix_shuffled": set()}


@pytest.mark.parametrize("case", C.SHELL_SOLVES, ids=lambda c: "-".join(map(str, c)))
def test_solver_bc_paths_on_a_shell_beyond_one_pass(case):
    """big_shell: the shell kernels of the solver loops (the BC fill between iterations, the shell term of the stop test)
    over two passes, on the default path of that BC set -- closed form, pair kernels or one launch per face -- and on every
    forced one: the oracle's result; fold 0 gives the bits of fold 1; and among the paths every bit of the iterate, the
    iteration count, tol and every scalar is the same.  One exemption: between a run on the pair kernels and one that is not,
    the stop-test value is held to summation order (1e-12, the bound of tests/test_gpu_bc_pair.py), because the pair kernels
    group the shell's share of that sum by axis and k_shell by pass (measured: one ulp)."""
    bc = case[2]
    bad = []
    runs = {path: _solve(case, fastpath=0, fold=1, **({} if path is None else {"bc_path": path})) for path in (None, 1, 3, 4)}
    _against_oracle(case, runs[None], "default path", bad)
    bad += [("default path, fold 0 vs fold 1", d) for d in _same_run(_solve(case, fastpath=0, fold=0), runs[None])]
    compared = 0
    for path in (1, 3, 4):
        a, b = runs[path], runs[None]
        print(f"{'-'.join(map(str, case))} bc_path {path}: tol {a[1]['tol']!r} (default path {b[1]['tol']!r})")
        if (path in PAIR_PATHS[bc]) != (None in PAIR_PATHS[bc]):
            for tol_a, tol_b in ((a[1]["tol"], b[1]["tol"]), (a[2]["tol"], b[2]["tol"])):
                if not abs(tol_a - tol_b) <= 1e-12 * abs(tol_b):
                    bad.append((f"bc_path {path} vs default", "tol beyond summation order", tol_a, tol_b))
            a = (a[0], dict(a[1], tol=b[1]["tol"]), dict(a[2], tol=b[2]["tol"]))
        bad += [(f"bc_path {path} vs default", d) for d in _same_run(a, b)]
        compared += 1
    assert compared == 3 and len(runs) == 4
    assert not bad, _told(bad)


@pytest.mark.parametrize("sweeps", [2, 3])
def test_save_old_beyond_one_pass(sweeps):
    """k_copy: after a Jacobi solve of an even and of an odd number of sweeps Field.VARo is the oracle's iterate one sweep
    earlier (at the solver's bound), and equals the tiled run's in every bit"""
    case = ("one_and_a_bit", "double", "mixv", "jacobi", sweeps)
    before = ("one_and_a_bit", "double", "mixv", "jacobi", sweeps - 1)
    assert case in C.GENERIC_SOLVES
    generic = _solve(case, save_old=True, fastpath=0)
    tiled = _solve(case, save_old=True, fastpath=1)
    xo, ro = C.oracle_solution(before) if before in C.GENERIC_SOLVES else _quiet(lambda: O.solve_poisson(
        C.omesh(case[0], case[1]), C.solve_cfgs(case, "cpu")[1], C.solve_inputs(case)[0].clone(), method="jacobi", tol=-1.0,
        max_it=sweeps - 2, coeff=0.7, sign=-1.0, omega=C.JACOBI_OMEGA))
    assert ro["itr"] == sweeps - 1
    assert generic[1]["itr"] == tiled[1]["itr"] == sweeps
    assert rel_err(generic[3], xo) <= 1e-10, rel_err(generic[3], xo)
    assert torch.equal(generic[3], tiled[3]) and torch.equal(generic[0], tiled[0])
    assert not torch.equal(generic[3], generic[0])


def _tiled_options(mid):
    return dict(C.TILED[mid][1], cg2d_mincells=-1)


@pytest.mark.parametrize("case", C.TILED_SOLVES, ids=lambda c: "-".join(map(str, c)))
def test_tiled_solvers_above_the_grid_cap(case):
    """one plane of more than 2048 tiles: the drivers leave the folded prologue for the single-block k_*_post kernels (on
    tiles_straddle in the full-extent phases only).  Against the oracle; against the generic kernels at the suite's
    tiled-versus-generic bounds (Jacobi: bit for bit); fold 1 against fold 0 bit for bit, iterate, itr, tol and scalars;
    BiCGSTAB with bicg_pfold 0 and 1, Jacobi with jac_alt 0 and 1."""
    mid, dtype, bc, method, iters = case
    opts = _tiled_options(mid)
    bad, ran = [], 0
    variants = {"cg": [{}], "bicgstab": [{"bicg_pfold": 1}, {"bicg_pfold": 0}], "jacobi": [{"jac_alt": 1}, {"jac_alt": 0}]}[method]
    generic = _solve(case, fastpath=0, **opts)
    _against_oracle(case, generic, "generic", bad)
    first = None
    for v in variants:
        tag = "tiled %s" % (v or "")
        folded = _solve(case, fastpath=1, fold=1, **opts, **v)
        plain = _solve(case, fastpath=1, fold=0, **opts, **v)
        _against_oracle(case, folded, tag, bad)
        bad += [(tag + " fold 1 vs fold 0", d) for d in _same_run(folded, plain)]
        _against_tiled(case, generic, folded, tag, bad)
        ran += 1
        if first is None:
            first = folded
        elif not torch.equal(folded[0], first[0]):
            bad.append((tag, "iterate differs from the first variant's", rel_err(folded[0], first[0])))
    assert ran == (1 if method == "cg" else 2)
    assert not bad, _told(bad)


def test_stepwise_cg_on_the_straddling_mesh():
    """tiles_straddle, cg_begin + three cg_iterate(1) + cg_end: every call ends on a flushed fold, with phases A / B folded
    and the A x phase not; the one-shot solve's bits"""
    from pyapes_amd.hip import lib as L
    case = ("tiles_straddle", "double", "dn", "cg", 3)
    assert case in C.TILED_SOLVES
    one_shot = _solve(case, fastpath=1, fold=1, **_tiled_options("tiles_straddle"))
    mesh, ctx = _mesh("tiles_straddle", "double", fastpath=1, fold=1, **_tiled_options("tiles_straddle"))
    dev_cfg, _ = C.solve_cfgs(case)
    var = Field("p", 1, mesh, {"domain": dev_cfg, "obstacle": None})
    rhs_d = C.solve_inputs(case)[0].cuda()
    ctx.bind_bcs(var(), var.bcs, 0, for_rhs=True)
    ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": 0.7}])
    ctx.rhs_adjust(rhs_d[0])
    ctx.bind_bcs(var(), var.bcs, 0)
    ctx.cg_begin(var()[0], rhs_d[0], -1.0, 1000)
    try:
        for _ in range(3):
            ctx.cg_iterate(1)
        rep = ctx.cg_end()
    except BaseException:
        ctx.cg_abort()
        raise
    assert int(rep.itr) == one_shot[1]["itr"] == 3
    assert torch.equal(var().cpu(), one_shot[0]), rel_err(var().cpu(), one_shot[0])
    assert float(rep.tol) == one_shot[1]["tol"]


# ---- the launch log ------------------------------------------------------------------------------------------------------------
def log_child(mid):
    """in a child process of its own (the launch log prints at most 8 lines per kernel instantiation and process, and the
    meshes share instantiations): one CG iteration, two BiCGSTAB iterations (the second forms v = A p in phase I) and two
    Jacobi sweeps (forwards, backwards) on one tiled mesh, a marker in front of each"""
    dtype = C.TILED[mid][0]
    for method, iters in (("cg", 1), ("bicgstab", 2), ("jacobi", 2)):
        torch.cuda.synchronize()
        sys.stderr.write("CASE %s %s\n" % (mid, method))
        sys.stderr.flush()
        _solve((mid, dtype, "dn", method, iters), fastpath=1, **_tiled_options(mid), **({"jac_alt": 1} if method == "jacobi" else {}))
    torch.cuda.synchronize()


def _blocks(lines):
    """{phase letter: [blocks of every launch line]} and the layout tags seen"""
    out, tags = {}, set()
    for ln in lines:
        m = re.search(r"k_cg3d phase (\w)((?: \([a-z]+\))?).*? blocks (\d+),", ln)
        if m:
            out.setdefault(m.group(1), []).append(int(m.group(3)))
            tags.add(m.group(2).strip())
    return out, tags


@pytest.mark.parametrize("mid", list(C.TILED))
def test_launch_log_shows_the_block_counts(mid):
    """the tile counts of grid_cap_cases are a prediction (rows per thread and blocks per CU come from the device): the
    launch log must show more than 2048 blocks in every phase of the tiles_above* meshes, and on tiles_straddle at most 2048
    in the interior phases (CG A, B; BiCGSTAB F, G, I) and more in the full-extent ones (A x: C; the Jacobi sweeps E, J)"""
    interior = {"cg": "AB", "bicgstab": "FGI", "jacobi": ""}
    required = {"cg": "C", "bicgstab": "", "jacobi": "EJ"}      # full-extent phases every run of the method must show
    ran = 0
    dtype, _, layout = C.TILED[mid]
    log = G.child("import test_gpu_grid_cap as T\nT.log_child(%r)\n" % mid, drop_options=True)
    seen = G.case_log(log, lambda ln: "[pyapes_hip]" in ln)
    for method in ("cg", "bicgstab", "jacobi"):
        blocks, tags = _blocks(seen["%s %s" % (mid, method)])
        print(mid, method, {k: sorted(set(v)) for k, v in sorted(blocks.items())}, sorted(tags))
        for ph in interior[method] + required[method]:
            assert ph in blocks, (mid, method, ph, blocks)
        assert not any("k_cg2d" in ln for ln in seen["%s %s" % (mid, method)])
        for ph, counts in blocks.items():
            if mid == "tiles_straddle" and ph in interior[method]:
                assert max(counts) <= C.PA_MAX_GRID, (mid, method, ph, counts)
                assert max(counts) == C.tiles(C.MESHES[mid][0], dtype, layout, True), (mid, method, ph, counts)
            else:
                assert min(counts) > C.PA_MAX_GRID, (mid, method, ph, counts)
            assert max(counts) <= C.PA_MAX_PARTIALS
        want = {"narrow": "(narrow)", "pitched": "(pitched)", "vector": ""}[layout]
        if method == "cg":       # the CG phases show the layout of their buffers
            assert want in tags and "(pitched)" not in (tags - {want}), (mid, method, tags)
        ran += 1
    assert ran == 3
