"""-m gpu: the kernels on signed zeros, subnormals, magnitudes next to the largest number and single non-finite cells -- the
fields of tests/edge_fields.py -- compared in BITS (helpers.same_bits: the integer views agree, -0 is not +0, a subnormal is
not 0, NaN is a class), tiled kernel against generic kernel and both against the CPU restatement tests/march_ref.py / the
oracle.  Single launches through the Context, outputs pre-filled with NaN.

A  finite classes (zeros, subnormal, large): the Euler step and a fused stage on k_sf (US 1 / 2 with a scalar speed of either
   sign, +0.0 and -0.0; HASU; SELF upwind and central; VEL; SRC), k_sfq (quick / minmod / mc), k_sfn (a nu field with its zero
   region), k_cg3d phase 3 (sf 0) and the generic k_euler; marches of three steps; the Euler march with BC on load.
B  the explicit operators, A x and one Jacobi sweep on the finite classes; the general Div in the literal upwind form with the
   AMBIGUOUS rule (tests/test_edge_fields_host.py: the cells at which the reference itself is not determinate in bits, which
   are compared by value).
C  one NaN, +inf or -inf at every named position (edge_fields.positions) of phi, of a stage's phi0, of a speed field, a
   velocity component, the source and nu; a scalar speed of NaN.

The documented exceptions (DESIGN.md section 4 "Edge values"), both pinned in their exact shape by C:
  * the US instantiations of k_sf / k_sfq leave out the half of every axis term whose speed half is zero.  Where that half's
    difference is not finite the literal form has 0 * (inf or NaN) = NaN and the US kernel a number;
  * the reference's five-point stencil sums carry two outer tables of zeros, which make NaN two nodes away from a non-finite
    cell of phi; the kernels read three points per axis and are held to the reference without those tables
    (edge_fields.three_point), from which the full reference may differ only where it has NaN.
"""
import warnings

import pytest
import torch

import edge_fields as E
import march_gpu as G
import march_ref as R
import pyapes_oracle as O
from helpers import same_bits
from pyapes_amd.hip.context import context_for
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import FDC
from pyapes_amd.solver.fdm import FDM
from pyapes_amd.solver.march import euler_march, momentum_march, rk_march
from pyapes_amd.solver.ops import Solver
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

STAGE = E.STAGE
CLASSES = ["zeros", "subnormal", "large"]
TILED_IDS = ["x".join(map(str, n)) + d[0] for n, d in E.TILED]
GENERIC_IDS = ["x".join(map(str, n)) + d[0] for n, d in E.GENERIC]
GENERIC_OPTS = {"fastpath": 0, "sf": 1, "sfq": 1, "chunks": 0}
DEFAULT_OPTS = {"fastpath": 1, "sf": 1, "sfq": 1, "chunks": 0}
# the tiled launches of a family: rows per wave 2 and 4, the chunk cap at 1 and 2; k_cg3d's phase 3 rides with k_sf (sf 0)
TILED_OPTS = {
    "k_sf": [{"fastpath": 1, "sf": sf, "sfq": 1, "chunks": ch} for sf in (2, 4, 0) for ch in (1, 2)],
    "k_sfq": [{"fastpath": 1, "sf": 1, "sfq": r, "chunks": ch} for r in (2, 4) for ch in (1, 2)],
    "k_sfn": [{"fastpath": 1, "sf": 1, "sfq": 1, "chunks": ch} for ch in (1, 2)],
}

_GPU = {}


def gpu(c):
    """the device side of a case of edge_fields.case: a mesh of its own (so: a context of its own) with the BCs bound, and
    device copies of the case's tensors"""
    key = (tuple(c["n"]), c["dtype"], c["bcname"], c["cls"])
    if key not in _GPU:
        nd = len(c["n"])
        mesh = Mesh(G.box(nd), None, list(c["n"]), "cuda", c["dtype"])
        bc = {"domain": mixed_bcs(c["vals"], c["types"]), "obstacle": None}
        ctx = context_for(mesh)
        f = Field("phi", 1, mesh, bc)
        ctx.bind_bcs(f(), f.bcs, 0)
        dev = {k: c[k].cuda() for k in ("phi", "phi0", "self_phi", "self_phi0", "speed", "nu_field", "src") if c[k] is not None}
        dev["vel"] = [t.cuda() for t in c["vel"]]
        _GPU[key] = dict(mesh=mesh, bc=bc, ctx=ctx, dev=dev, bound=f)
    return _GPU[key]


def set_options(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)


def launch(c, form, stage, opts, **over):
    """one Euler step (``stage`` None) or fused stage of ``form`` with the options ``opts``; ``over``: CPU replacements of the
    case's tensors (edge_fields.operands).  Returns the (1, *n) result on the CPU."""
    g = gpu(c)
    ctx = g["ctx"]
    set_options(ctx, opts)
    dev = dict(g["dev"])
    for k, v in over.items():
        dev[k] = [t.cuda() for t in v] if k == "vel" else v.cuda()
    fam, lim, u, with_src, nuf = E.FORMS[form]
    own = u == "self" and "self_phi" in dev
    phi, phi0 = (dev["self_phi"], dev["self_phi0"]) if own else (dev["phi"], dev["phi0"])
    out = torch.full_like(phi, float("nan"))
    kind = G.kind(lim)
    src = dev["src"][0] if with_src else None
    p0 = None if stage is None else phi0[0]
    c0, c1 = stage or (0.0, 0.0)
    if u == "vel":
        speed = list(dev["vel"])
    else:
        speed = {"field": dev["speed"][0], "self": phi[0]}.get(u, u) if isinstance(u, str) else u
    if nuf:
        ctx.step_nu(phi[0], p0, out[0], c0, c1, kind, speed, dev["nu_field"], c["dt"], source=src)
    elif u == "vel":
        if stage is None:
            ctx.euler_step_vel(phi[0], out[0], kind, speed, c["nu"], c["dt"], source=src)
        else:
            ctx.rk_stage_vel(phi[0], p0, out[0], c0, c1, kind, speed, c["nu"], c["dt"], source=src)
    elif stage is None:
        ctx.euler_step(phi[0], out[0], kind, speed, c["nu"], c["dt"], source=src)
    else:
        ctx.rk_stage(phi[0], p0, out[0], c0, c1, kind, speed, c["nu"], c["dt"], source=src)
    return out.cpu()


def told(bad):
    return "%d differ; the first: %s" % (len(bad), " | ".join(repr(b) for b in bad[:4]))


def differ(a, b):
    """the cells at which ``a`` and ``b`` do not hold the same bits (NaN as a class)"""
    na, nb = torch.isnan(a), torch.isnan(b)
    bits = torch.int32 if a.dtype == torch.float32 else torch.int64
    return (na != nb) | (~na & ~nb & (a.view(bits) != b.view(bits)))


@pytest.fixture(autouse=True)
def _default_options_afterwards():
    yield
    for g in _GPU.values():
        set_options(g["ctx"], DEFAULT_OPTS)
        g["ctx"].set_option("bcl", 1)


# ---- A. the finite classes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bcname", ["dir", "mix", "xper", "zper"])
@pytest.mark.parametrize("family", ["k_sf", "k_sfq", "k_sfn"])
@pytest.mark.parametrize("n,dtype", E.TILED, ids=TILED_IDS)
@pytest.mark.parametrize("cls", CLASSES)
def test_finite_step_and_stage_tiled_generic_reference(cls, n, dtype, family, bcname):
    bad, launches = [], 0
    c = E.case(n, dtype, bcname, cls)
    for form in E.family_forms(family):
        if bcname not in E.form_bcs(form):
            continue
        for stage in (None, STAGE):
            want = E.reference(c, form, stage)
            assert bool(torch.isfinite(want).all())
            gen = launch(c, form, stage, GENERIC_OPTS)
            r = same_bits(gen, want)
            if not r:
                bad.append((form, stage, "generic vs reference", r.why))
            for opts in TILED_OPTS[family]:
                got = launch(c, form, stage, opts)
                launches += 1
                r = same_bits(got, gen)
                if not r:
                    bad.append((form, stage, opts, "tiled vs generic", r.why))
    assert launches > 0 and not bad, told(bad)


@pytest.mark.parametrize("n,dtype", E.GENERIC, ids=GENERIC_IDS)
@pytest.mark.parametrize("cls", CLASSES)
def test_finite_step_and_stage_generic_kernel(cls, n, dtype):
    """k_euler on the 1-D / 2-D / odd meshes, every form (the NU instantiation: the sfn forms)"""
    bad = []
    for form in E.FINITE_FORMS:
        for bcname in E.form_bcs(form):
            if bcname == "zper" and len(n) < 3:
                continue
            c = E.case(n, dtype, bcname, cls)
            for stage in (None, STAGE):
                want = E.reference(c, form, stage)
                r = same_bits(launch(c, form, stage, DEFAULT_OPTS), want)
                if not r:
                    bad.append((form, bcname, stage, r.why))
    assert not bad, told(bad)


MARCH_MESHES = [([10, 12, 132], "double"), ([6, 7, 260], "single")]


def _march_field(c, t):
    g = gpu(c)
    return G.fresh_field(g["mesh"], g["bc"], t)


@pytest.mark.parametrize("n,dtype", MARCH_MESHES, ids=["10x12x132d", "6x7x260s"])
@pytest.mark.parametrize("cls", CLASSES)
def test_finite_marches_of_three_steps(cls, n, dtype):
    """rk_march of order 3 (a speed field, QUICK with a scalar speed) and momentum_march, three steps each, and the Euler
    march with and without BC on load: the bits of march_ref"""
    c = E.case(n, dtype, "mix", cls)
    g = gpu(c)
    set_options(g["ctx"], DEFAULT_OPTS)
    for lim, u_ref, u_dev in (("upwind", c["speed"], g["dev"]["speed"]), ("quick", -0.7, -0.7)):
        f = _march_field(c, c["phi"])
        rk_march(f, u_dev, c["nu"], c["dt"], 3, G.config(lim), order=3)
        want = R.march(c["phi"], u_ref, c["nu"], c["dt"], 3, c["om"], c["obcs"], lim, 3)
        assert bool(torch.isfinite(want).all())
        assert same_bits(f(), want), (lim, same_bits(f(), want).why)
    want = R.march(c["phi"], 0.7, c["nu"], c["dt"], 3, c["om"], c["obcs"], "upwind", 1)
    for bcl in (0, 1):
        g["ctx"].set_option("bcl", bcl)
        f = _march_field(c, c["phi"])
        euler_march(f, 0.7, c["nu"], c["dt"], 3, G.config("upwind"))
        assert same_bits(f(), want), (bcl, same_bits(f(), want).why)
    # the vector field, three fields of the class as its components: it advects itself -- class "large": in the frozen O(1)
    # velocity of the class (the linearised form), since a product of two of its own values is not finite
    U = torch.cat([c[k] for k in ("phi", "phi0", "src")]).clone()
    for q in range(3):
        O.bc_fill(U[q:q + 1], c["obcs"])
    u_ref, u_dev = (list(c["vel"]), torch.stack(g["dev"]["vel"])) if cls == "large" else (None, None)
    f = _march_field(c, U)
    momentum_march(f, c["nu"], c["dt"], 3, G.config("upwind"), order=3, u=u_dev)
    want = R.momentum.march(U, c["nu"], c["dt"], 3, c["om"], [c["obcs"]] * 3, "upwind", 3, None, u_ref)
    assert bool(torch.isfinite(want).all())
    assert same_bits(f(), want), same_bits(f(), want).why


# ---- B. the explicit operators, A x and a Jacobi sweep ----------------------------------------------------------------------
def _explicit(c, fast):
    """{name: CPU result} of the explicit operators, A x of a one-term and a two-term equation and one Jacobi sweep on the
    case's phi with its speed field, on the tiled (``fast``) or the generic kernels"""
    g = gpu(c)
    set_options(g["ctx"], dict(DEFAULT_OPTS, fastpath=int(fast)))
    var = _march_field(c, c["phi"])
    speed = g["dev"]["speed"]
    res = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res["lap"] = FDC({"laplacian": {"edge": False}}).laplacian(var).cpu()
        res["grad"] = FDC({"grad": {"edge": False}}).grad(var).cpu()
        lims = ["upwind", "quick", "minmod", "mc", "compat"] + (["none"] if c["bcname"] != "mix" else [])
        for lim in lims:
            cfg = {"div": {"limiter": "upwind" if lim == "compat" else lim, "compat": lim == "compat", "edge": False}}
            res["div_" + lim] = FDC(cfg).div(speed, var).cpu()
            if lim in ("upwind", "quick"):
                for tag, u in (("pos", 0.7), ("neg", -0.7), ("negzero", -0.0)):
                    res["div_%s_%s" % (lim, tag)] = FDC(cfg).div(u, var).cpu()
        solver = Solver({"fdm": {"method": "cg", "tol": 1e-6, "max_it": 1, "report": False}})
        solver.set_eq(-FDM().laplacian(0.7, var) == torch.zeros_like(var()))
        res["aop_one"] = solver.Aop(var).cpu()
        solver = Solver({"fdm": {"method": "bicgstab", "tol": 1e-6, "max_it": 1, "report": False}})
        solver.set_eq(FDM({"div": {"limiter": "upwind", "compat": True}}).div(speed, var) - FDM().laplacian(0.05, var)
                      == torch.zeros_like(var()))
        res["aop_two"] = solver.Aop(var).cpu()
        for resident in (0, 1):
            g["ctx"].set_option("resident", resident)
            # (class "large": the stop test squares the residual, so the sweep takes the fields of square-root magnitude)
            x0, rhs = (c["phi0"], g["dev"]["src"]) if c["self_phi"] is None else (c["self_phi0"] * 2.0 ** -24, g["dev"]["self_phi"])
            x = _march_field(c, x0)
            solver = Solver({"fdm": {"method": "jacobi", "tol": 1e-30, "max_it": 0, "report": False, "omega": 0.9}})
            solver.set_eq(FDM().laplacian(0.8, x) == rhs.clone())
            solver.solve()
            res["jacobi_resident%d" % resident] = x().cpu()
    return res


def _explicit_reference(c):
    phi, speed, om, obcs, nd = c["phi"], c["speed"], c["om"], c["obcs"], len(c["n"])
    ref = {"lap": O.apply_laplacian(O.laplacian_tables(phi, om, obcs), phi, nd),
           "grad": O.apply_grad(O.grad_tables(phi, om, obcs), phi, nd),
           "div_upwind": O.div_upwind_intended(speed, phi, om), "div_quick": R.div_quick(speed, phi, om, obcs),
           "div_minmod": R.div_tvd(speed, phi, om, obcs, "minmod"), "div_mc": R.div_tvd(speed, phi, om, obcs, "mc"),
           "div_compat": E.general_div(c)}
    if c["bcname"] != "mix":
        ref["div_none"] = O.apply_div(O.div_tables(speed, phi, om, obcs, "none"), phi, nd)
    for tag, u in (("pos", 0.7), ("neg", -0.7), ("negzero", -0.0)):
        ref["div_upwind_" + tag] = O.div_upwind_intended(u, phi, om)
        ref["div_quick_" + tag] = R.div_quick(u, phi, om, obcs)
    # A x of  -laplacian(0.7, phi)  and of  div(speed, phi) - laplacian(0.05, phi)  (the literal upwind Div)
    one = [{"kind": "laplacian", "sign": -1.0, "coeff": 0.7}]
    two = [{"kind": "div", "sign": 1.0, "u": speed, "limiter": "upwind"}, {"kind": "laplacian", "sign": -1.0, "coeff": 0.05}]
    ref["aop_one"] = O.Aop(phi, O.equation_terms(om, obcs, one, phi)[0], nd)
    ref["aop_two"] = O.Aop(phi, O.equation_terms(om, obcs, two, phi)[0], nd)
    # one Jacobi sweep of  laplacian(0.8, x) == rhs  from the x0 and rhs of _explicit
    x0, rhs = (c["phi0"], c["src"]) if c["self_phi"] is None else (c["self_phi0"] * 2.0 ** -24, c["self_phi"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sweep, _ = O.solve_poisson(om, O.mixed_cfg(c["vals"], c["types"], O.FACES[:2 * nd]), rhs.clone(), x0.clone(), method="jacobi",
                                   tol=1e-30, max_it=0, coeff=0.8, omega=0.9)
    ref["jacobi_resident0"] = ref["jacobi_resident1"] = sweep
    return ref


@pytest.mark.parametrize("bcname", ["dir", "mix", "zper"])
@pytest.mark.parametrize("n,dtype", [E.TILED[1], E.TILED[3]] + E.GENERIC, ids=["10x12x132d", "9x14x260s"] + GENERIC_IDS)
@pytest.mark.parametrize("cls", CLASSES)
def test_explicit_operators_aop_and_jacobi(cls, n, dtype, bcname):
    """tiled against generic in every bit; laplacian, grad and every Div against the oracle / march_ref, the general Div
    under the AMBIGUOUS rule"""
    if bcname == "zper" and len(n) < 3:
        bcname = "xper"
    c = E.case(n, dtype, bcname, cls)
    fast, slow = _explicit(c, True), _explicit(c, False)
    bad = []
    for k in fast:
        r = same_bits(fast[k], slow[k])
        if not r:
            bad.append((k, "tiled vs generic", r.why))
    r = same_bits(fast["jacobi_resident0"], fast["jacobi_resident1"])
    if not r:
        bad.append(("jacobi", "resident 0 vs 1", r.why))
    ref = _explicit_reference(c)
    mask, ok = E.ambiguous(E.reference_variants(c, lambda **over: E.general_div(c, **over)))
    assert ok and 16 * int(mask.sum()) <= mask.numel()
    for k, want in ref.items():
        got = fast[k].reshape(want.shape)
        if k == "div_compat" and bool(mask.any()):
            r = same_bits(torch.where(mask, torch.zeros_like(got), got), torch.where(mask, torch.zeros_like(want), want))
            if not (r and torch.equal(got[mask], want[mask])):
                bad.append((k, "vs reference off / on the AMBIGUOUS cells", r.why))
            continue
        r = same_bits(got, want)
        if not r:
            bad.append((k, "vs reference", r.why))
    assert not bad, told(bad)


# ---- C. non-finite cells ------------------------------------------------------------------------------------------------
C_FORMS = ["sf_up_pos", "sf_up_neg", "sf_up_field", "sf_self_cen", "sf_vel", "sf_src", "sfq_quick_pos", "sfq_minmod_neg",
           "sfq_mc_field", "sfq_quick_self", "sfn_neg"]
C_GENERIC_FORMS = ["sf_up_pos", "sf_up_field", "sf_self_cen", "sfq_mc_field", "sfn_neg"]


def _neighbours(at, n, sign):
    """the nodes that read the node ``at`` through the LIVE half of a scalar speed of sign ``sign``, inside the interior set"""
    out = []
    for a in range(len(n)):
        p = list(at)
        p[a] += sign
        if all(1 <= i <= m - 2 for i, m in zip(p, n)):
            out.append(tuple(p))
    return out


def is_us_launch(fam, opts):
    """the launch runs a US instantiation of k_sf / k_sfq (sf 0 is k_cg3d phase 3, sfq 0 the generic kernel: both halves)"""
    return bool(opts.get("fastpath", 1)) and ((fam == "k_sf" and opts["sf"] != 0) or (fam == "k_sfq" and opts["sfq"] != 0))


def check_us_exception(c, form, phi, got, gen, cells, bad, tag):
    """the documented exception: tiled and generic differ only where the left-out half's difference is not finite, the
    generic kernel has NaN there, and the planted cells and their live-side neighbours are non-finite on both"""
    d = differ(got, gen)
    dead = E.through_bc_fill(E.dead_half_nonfinite(c, form, phi), c)
    if bool((d & ~dead).any()):
        bad.append(tag + ("differs off the dead side", same_bits(torch.where(dead, gen, got), gen).why))
    if not bool(torch.isnan(gen[d]).all()):
        bad.append(tag + ("the generic kernel has a number where the US kernel differs",))
    n = c["n"]
    for at in cells:
        near = ([at] if all(1 <= i <= m - 2 for i, m in zip(at, n)) else []) + _neighbours(at, n, E.us_sign(form))
        for p in near:
            if bool(torch.isfinite(got[(0, *p)])) or bool(torch.isfinite(gen[(0, *p)])):
                bad.append(tag + ("finite at", p, float(got[(0, *p)]), float(gen[(0, *p)])))


def planted_phi_and_phi0(c, form, tiled_opts, generic_opts):
    """every position x NaN / +inf / -inf in phi of a step and in phi0 of a stage"""
    bad = []
    n, fam = c["n"], E.FORMS[form][0]
    e_clean = E.reference(c, form, None)
    for names, at in E.distinct_positions(n, c["dtype"]):
        for value in E.NONFINITE:
            tag = (form, names, value)
            # in phi of a step
            phi_p = E.planted(c["phi"], value, at)
            want = E.reference(c, form, None, phi=phi_p)
            with E.three_point():
                want3 = E.reference(c, form, None, phi=phi_p)
            if not bool(torch.isnan(want[differ(want3, want)]).all()):
                bad.append(tag + ("phi: the five-point reference has a number where the three-point one differs",))
            gen = launch(c, form, None, generic_opts, phi=phi_p)
            r = same_bits(gen, want3)
            if not r:
                bad.append(tag + ("phi: generic vs three-point reference", r.why))
            if bool(torch.isfinite(want[(0, *at)])) and names.find("boundary") < 0:
                bad.append(tag + ("phi: the reference is finite at the planted cell",))
            for opts in tiled_opts:
                got = launch(c, form, None, opts, phi=phi_p)
                if E.us_sign(form) and is_us_launch(fam, opts):
                    check_us_exception(c, form, phi_p, got, gen, [at], bad, tag + (str(opts),))
                else:
                    r = same_bits(got, gen)
                    if not r:
                        bad.append(tag + (str(opts), "phi: tiled vs generic", r.why))
            # in phi0 of a stage (the Euler value of the stage is the clean one)
            phi0_p = E.planted(c["phi0"], value, at)
            want = E.reference(c, form, STAGE, e=e_clean, phi0=phi0_p)
            if bool(torch.isfinite(want[(0, *at)])) and names.find("boundary") < 0:
                bad.append(tag + ("phi0: the reference is finite at the planted cell",))
            for opts in [generic_opts] + list(tiled_opts):
                got = launch(c, form, STAGE, opts, phi0=phi0_p)
                r = same_bits(got, want)
                if not r:
                    bad.append(tag + (str(opts), "phi0: vs reference", r.why))
    return bad


@pytest.mark.parametrize("form", C_FORMS)
@pytest.mark.parametrize("n,dtype", E.TILED, ids=TILED_IDS)
def test_nonfinite_cell_in_phi_and_phi0_tiled(n, dtype, form):
    sets = E.form_bcs(form)
    bcname = sets[E.TILED.index((n, dtype)) % len(sets)]
    c = E.case(n, dtype, bcname, "plain")
    bad = planted_phi_and_phi0(c, form, TILED_OPTS[E.FORMS[form][0]], GENERIC_OPTS)
    assert not bad, told(bad)


@pytest.mark.parametrize("form", C_GENERIC_FORMS)
@pytest.mark.parametrize("n,dtype", E.GENERIC, ids=GENERIC_IDS)
def test_nonfinite_cell_in_phi_and_phi0_generic_kernel(n, dtype, form):
    sets = [b for b in E.form_bcs(form) if b != "zper" or len(n) == 3]
    c = E.case(n, dtype, sets[E.GENERIC.index((n, dtype)) % len(sets)], "plain")
    bad = planted_phi_and_phi0(c, form, [], DEFAULT_OPTS)
    assert not bad, told(bad)


@pytest.mark.parametrize("form", [f for f in E.FINITE_FORMS if E.us_sign(f)])
@pytest.mark.parametrize("n,dtype", [E.TILED[1], E.TILED[3]], ids=["10x12x132d", "9x14x260s"])
def test_overflowing_difference_on_the_us_kernels(n, dtype, form):
    """two finite neighbours of opposite sign above half the largest number: their difference overflows.  "Every finite
    field gives the same bits" is too strong; what holds is "every finite dead-side difference"."""
    bad = []
    for bcname in ("dir", "mix"):
        c = E.case(n, dtype, bcname, "overflow")
        cells = c["planted"]["cells"]
        for stage in (None, STAGE):
            want = E.reference(c, form, stage)
            assert int(torch.isnan(want).sum()) >= 1
            gen = launch(c, form, stage, GENERIC_OPTS)
            r = same_bits(gen, want)
            if not r:
                bad.append((form, bcname, stage, "generic vs reference", r.why))
            for opts in TILED_OPTS[E.FORMS[form][0]]:
                got = launch(c, form, stage, opts)
                if is_us_launch(E.FORMS[form][0], opts):
                    check_us_exception(c, form, c["phi"], got, gen, cells, bad, (form, bcname, stage, str(opts)))
                else:
                    r = same_bits(got, gen)
                    if not r:
                        bad.append((form, bcname, stage, str(opts), "tiled vs generic", r.why))
    assert not bad, told(bad)


# a NaN and an inf in a speed field, one velocity component, the source and nu: (form, the tensor that takes the cell)
OPERAND_CASES = [("sf_up_field", "speed"), ("sfq_quick_field", "speed"), ("sfq_mc_field", "speed"), ("sf_vel", "vel"),
                 ("sf_src", "src"), ("sf_src_field", "speed"), ("sf_src_field", "src"), ("sfn_neg", "nu_field"),
                 ("sfn_u0", "nu_field")]
OPERAND_POSITIONS = ("interior", "vector_last", "vector_first", "strip_last", "strip_first", "rows_first", "chunk_first",
                     "axis0_1", "axis2_n2", "boundary")


@pytest.mark.parametrize("form,operand", OPERAND_CASES, ids=["%s-%s" % fo for fo in OPERAND_CASES])
@pytest.mark.parametrize("n,dtype", E.TILED, ids=TILED_IDS)
def test_nonfinite_cell_in_speed_velocity_source_and_nu(n, dtype, form, operand):
    """the bits and the NaN mask of march_ref on the tiled and the generic kernels: a NaN speed is NOT "no flow" """
    sets = E.form_bcs(form)
    c = E.case(n, dtype, sets[E.TILED.index((n, dtype)) % len(sets)], "plain")
    pos = E.positions(n, dtype)
    bad = []
    comp = len(n) - 1
    for name in OPERAND_POSITIONS:
        if name not in pos:
            continue
        for value in ("nan", "+inf"):
            if operand == "vel":
                over = {"vel": [E.planted(t, value, pos[name]) if a == comp else t for a, t in enumerate(c["vel"])]}
            else:
                over = {operand: E.planted(c[operand], value, pos[name])}
            for stage in (None, STAGE):
                want = E.reference(c, form, stage, **over)
                if name != "boundary" and bool(torch.isfinite(want[(0, *pos[name])])):
                    bad.append((name, value, stage, "the reference is finite at the planted cell"))
                for opts in [GENERIC_OPTS] + TILED_OPTS[E.FORMS[form][0]]:
                    r = same_bits(launch(c, form, stage, opts, **over), want)
                    if not r:
                        bad.append((name, value, stage, str(opts), r.why))
    assert not bad, told(bad)


@pytest.mark.parametrize("value", ["finite", "nan", "+inf"])
@pytest.mark.parametrize("n,dtype", [E.TILED[1], ([7, 15, 132], "double"), E.TILED[3]], ids=["10x12x132d", "7x15x132d", "9x14x260s"])
def test_march_with_a_speed_field_and_a_source_on_load_and_classic(n, dtype, value):
    """rk_march of order 3 with a speed field AND a source on dirichlet / mixed scalar faces: with ``bcl`` 1 the Euler launches
    and the stages run the BC-on-load SRC instantiations of k_sf (pa_sf_src_bcl.hip; forced to four rows per wave, where the
    fp64 stage with a speed field has a two-row instantiation only), with ``bcl`` 0 the classic ones, with ``fastpath`` 0 the
    generic kernel.  On 15 rows (n1 - 1 even) the two-row stage declines BC on load after the four-row Euler launch took it:
    the march goes on in the classic sequence.  A NaN / inf in the speed must come out as in march_ref on all of them: within one march no launch may
    propagate it and the next swallow it."""
    bad = []
    for bcname in ("dir", "mix"):
        c = E.case(n, dtype, bcname, "plain")
        g = gpu(c)
        pos = E.positions(n, dtype)
        for name in (("interior",) if value == "finite" else ("interior", "strip_first", "rows_first", "axis0_1")):
            u = c["speed"] if value == "finite" else E.planted(c["speed"], value, pos[name])
            with E.three_point():   # (from the second launch on phi holds the non-finite cells: the kernels' three points)
                want = R.march(c["phi"], u, c["nu"], c["dt"], 2, c["om"], c["obcs"], "upwind", 3, c["src"])
            assert value == "finite" or int((~torch.isfinite(want)).sum()) >= 1
            for opts in ({"fastpath": 0}, {"fastpath": 1, "sf": 4, "bcl": 1}, {"fastpath": 1, "sf": 2, "bcl": 1},
                         {"fastpath": 1, "sf": 4, "bcl": 0}, {"fastpath": 1, "sf": 1, "bcl": 1}):
                set_options(g["ctx"], dict(DEFAULT_OPTS, **opts))
                f = _march_field(c, c["phi"])
                rk_march(f, u.cuda(), c["nu"], c["dt"], 2, G.config("upwind"), order=3, source=g["dev"]["src"])
                r = same_bits(f(), want)
                if not r:
                    bad.append((bcname, name, value, opts, r.why))
    assert not bad, told(bad)


@pytest.mark.parametrize("n,dtype", [E.TILED[1], E.TILED[3], E.GENERIC[0]], ids=["10x12x132d", "9x14x260s", "6x7x9d"])
def test_nonfinite_speed_in_the_explicit_div(n, dtype):
    c = E.case(n, dtype, "mix", "plain")
    g = gpu(c)
    pos = E.positions(n, dtype)
    bad = []
    refs = {"upwind": lambda u: O.div_upwind_intended(u, c["phi"], c["om"]),
            "quick": lambda u: R.div_quick(u, c["phi"], c["om"], c["obcs"]),
            "mc": lambda u: R.div_tvd(u, c["phi"], c["om"], c["obcs"], "mc"),
            "compat": lambda u: E.general_div(c, speed=u)}
    for name in ("interior", "strip_first", "axis0_1"):
        if name not in pos:
            continue
        for value in ("nan", "+inf"):
            u = E.planted(c["speed"], value, pos[name])
            for lim, ref in refs.items():
                want = ref(u)
                assert int((~torch.isfinite(want)).sum()) >= 1
                cfg = {"div": {"limiter": "upwind" if lim == "compat" else lim, "compat": lim == "compat", "edge": False}}
                for fast in (1, 0):
                    set_options(g["ctx"], dict(DEFAULT_OPTS, fastpath=fast))
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        got = FDC(cfg).div(u.cuda(), _march_field(c, c["phi"])).cpu()
                    r = same_bits(got, want)
                    if not r:
                        bad.append((name, value, lim, "fastpath %d" % fast, r.why))
    assert not bad, told(bad)


@pytest.mark.parametrize("form", E.NAN_SPEED_FORMS)
@pytest.mark.parametrize("n,dtype", [E.TILED[0], E.TILED[3], E.GENERIC[1]], ids=["14x12x16d", "9x14x260s", "17x12d"])
def test_scalar_speed_of_nan_gives_the_reference(n, dtype, form):
    """the library takes a NaN speed like any other number: NaN at every node of the interior set, the faces filled"""
    fam = E.FORMS[form][0]
    c = E.case(n, dtype, "mix", "plain")
    for stage in (None, STAGE):
        want = E.reference(c, form, stage)
        assert int(torch.isnan(want).sum()) >= 1
        for opts in [GENERIC_OPTS] + (TILED_OPTS[fam] if len(n) == 3 else []):
            r = same_bits(launch(c, form, stage, opts), want)
            assert r, (stage, opts, r.why)
