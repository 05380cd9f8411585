"""-m gpu: the QUICK advection scheme, Div limiter "quick" (PA_OP_DIV_QUICK: the generic kernels of csrc/pa_device.h, the
marching kernel k_sfq of csrc/pa_sfq_kernel.h).

The yardstick of the BITS is tests/march_ref.py, the torch-CPU restatement of the definition: FDC.div at every node and one
euler_step must equal it bit for bit, fp32 and fp64, on k_sfq and on the generic kernel.  A fused Runge-Kutta stage must be
euler_step + three torch ops + apply_bcs, the march must be its stages, no kernel switch may change a bit, and the facts
tests/test_quick_host.py establishes on the CPU must hold through rk_march on the GPU with the same bounds.

(The 5-node rule: an axis of 4 nodes is refused, PA_E_ARG -- x[-2] and x[+2] would be one node.  The few-rows-per-wave case on
four rows of nodes that the other march suites use, [16, 4, 32], therefore appears here among the ERRORS, and [16, 5, 32]
stands in for it among the k_sfq cases: the smallest row count that runs, halo rows +-2 wrapping inside the tile.)
"""
import pytest
import torch

import march_gpu as G
import march_ref as Q
import pyapes_oracle as O
import test_gpu_rk as R
import test_quick_host as H
import test_self_march_host as HS
from helpers import bit_equal, offset_view
from march_gpu import XPER
from pyapes_amd.geometry import Box, Cylinder
from pyapes_amd.hip import lib as L
from pyapes_amd.hip.context import context_for
from pyapes_amd.hip.lib import PaError
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import FDC
from pyapes_amd.solver.march import euler_march, euler_step, rk_march, rk_step
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

QUICK = {"div": {"limiter": "quick"}}

# name, n, dtype, bcs, u ("field": a randn speed tensor, "self": the field itself), operands misaligned, context options,
# the kernel the Euler step must run on
CASES = [
    ("sfq_f32_config4", [40, 36, 72], "single", R.NEUSYM, 1.0, False, {}, "k_sfq"),
    ("sfq_f64_allneu_uneg", [24, 20, 66], "double", R.ALLNEU, -0.8, False, {}, "k_sfq"),
    ("sfq_f64_mixed", [21, 19, 34], "double", R.MIXED, 0.6, False, {}, "k_sfq"),
    ("sfq_f32_speed_field", [20, 24, 64], "single", R.NEUSYM, "field", False, {}, "k_sfq"),        # both signs in one row
    ("sfq_f64_two_ktiles_field", [12, 20, 136], "double", R.ALLDIR, "field", False, {}, "k_sfq"),  # the edge-cell pairs
    ("sfq_f32_two_ktiles", [9, 40, 264], "single", R.ALLDIR, 1.3, False, {}, "k_sfq"),
    ("sfq_f64_six_rows", [80, 6, 32], "double", R.MIXED, 1.0, False, {}, "k_sfq"),                 # halo rows wrap in the tile
    ("sfq_f64_five_rows", [16, 5, 32], "double", R.MIXED, -1.0, False, {}, "k_sfq"),
    ("sfq_f64_short_chunks_upos", [6, 12, 32], "double", R.ALLDIR, 1.0, False, {}, "k_sfq"),       # six planes: both axis-0 fallback pairs adjacent (chunks of ONE plane, like every
                                                                                                   # case here: 256 CUs x 2 blocks >= tiles x n0; longer chunks: test_gpu_chunks.py)
    ("sfq_f64_short_chunks_uneg", [6, 12, 32], "double", R.ALLDIR, -1.0, False, {}, "k_sfq"),
    ("sfq_f64_yperiodic", [16, 20, 40], "double", R.YPER, -1.1, False, {}, "k_sfq"),               # (stage: + k_rk_combine)
    ("sfq_f32_kperiodic", [12, 16, 64], "single", R.DIRPER, 1.2, False, {}, "k_sfq"),
    ("sfq_f64_self", [21, 19, 34], "double", R.MIXED, "self", False, {}, "k_sfq"),
    ("sfq_f32_self", [40, 36, 72], "single", R.NEUSYM, "self", False, {}, "k_sfq"),
    ("gen_f32_odd_rows", [17, 19, 33], "single", R.MIXED, 0.9, False, {}, "k_euler"),
    ("gen_f64_2d", [33, 48], "double", R.MIX2D, -0.7, False, {}, "k_euler"),
    ("gen_f64_1d", [65], "double", R.MIX1D, 0.8, False, {}, "k_euler"),
    ("gen_f32_1d_periodic", [64], "single", R.PER1D, -1.0, False, {}, "k_euler"),
    ("gen_f64_xperiodic", [16, 20, 40], "double", XPER, 0.7, False, {}, "k_euler"),
    ("gen_f64_xperiodic_field", [16, 20, 40], "double", XPER, "field", False, {}, "k_euler"),
    ("gen_f32_misaligned", [40, 36, 72], "single", R.NEUSYM, 1.0, True, {}, "k_euler"),
    ("gen_f32_sf_off", [40, 36, 72], "single", R.NEUSYM, 1.0, False, {"sf": 0}, "k_euler"),
    ("gen_f32_fastpath_off", [40, 36, 72], "single", R.NEUSYM, 1.0, False, {"fastpath": 0}, "k_euler"),
    ("gen_f32_sfq_off", [40, 36, 72], "single", R.NEUSYM, 1.0, False, {"sfq": 0}, "k_euler"),
    ("gen_f64_sfq_off_field", [12, 20, 136], "double", R.ALLDIR, "field", False, {"sfq": 0}, "k_euler"),
]
CASE = {c[0]: c for c in CASES}
NAMES = [c[0] for c in CASES]
SFQ_NAMES = [c[0] for c in CASES if c[-1] == "k_sfq"]


def _setup(name, seed=13):
    """test_gpu_rk._setup on this module's cases: mesh, BC config, (phi_s, phi0) BC-filled, the speed, nu, dt.  A misaligned
    case hands out BOTH fields as contiguous views one element into a larger allocation."""
    _, n, dtype, bcs, u, misaligned, options, kernel = CASE[name]
    key = "_quick_" + name
    R.CASE[key] = (key, n, dtype, bcs, QUICK, "field" if u in ("field", "self") else u, misaligned, options, kernel)
    try:
        mesh, bc, _, phis, phi0, uu, nu, dt = R._setup(key, seed)
    finally:
        del R.CASE[key]
    if misaligned:
        shape, values = phis.shape, phis.clone()
        phis, _ = offset_view(phis, 1)
        assert phis.is_contiguous() and phis.data_ptr() % 16 != 0
        assert phis.shape == shape and phis.is_cuda and torch.equal(phis, values)
    if u == "self":
        uu = phis
    return mesh, bc, phis, phi0, uu, nu, dt


def _oracle_side(name, mesh):
    _, n, dtype, bcs, *_ = CASE[name]
    nd = len(n)
    om = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
    ob = O.make_bcs(om, O.mixed_cfg(list(bcs[0]), list(bcs[1]), O.FACES[:2 * nd]))
    return om, ob


# ---- 1. bits against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_div_and_euler_step_are_the_restatement_bit_for_bit(name):
    mesh, bc, phis, _, u, nu, dt = _setup(name)
    om, ob = _oracle_side(name, mesh)
    x = phis.cpu().clone()
    uc = u.cpu().clone() if isinstance(u, torch.Tensor) else u
    f = G.fresh_field(mesh, bc, phis)
    if phis.data_ptr() % 16 != 0:
        f.set_var_tensor(phis)                       # keep the misaligned storage
    d = FDC(QUICK).div(u if not isinstance(u, torch.Tensor) else u.clone(), f)
    ref = Q.div_quick(uc, x, om, ob)
    assert bool(torch.isfinite(ref).all())
    assert bit_equal(d, ref), ("div", float((d.cpu() - ref).abs().max()), int((d.cpu() != ref).sum()))
    ctx = context_for(mesh)
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.full_like(phis, float("nan"))
    ctx.euler_step(phis[0], out[0], L.OP_DIV_QUICK, u, nu, dt)     # (u is phis itself in the self cases)
    ref = Q.euler_step(x, uc, nu, dt, om, ob, "quick")
    assert bit_equal(out, ref), ("euler_step", float((out.cpu() - ref).abs().max()), int((out.cpu() != ref).sum()))
    g = euler_step(G.fresh_field(mesh, bc, phis), u, nu, dt, QUICK)     # the public entry
    assert bit_equal(g(), ref)


def _step_and_stage(name):
    mesh, bc, phis, phi0, u, nu, dt = _setup(name)
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, phis)
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.empty_like(phis)
    ctx.euler_step(phis[0], out[0], L.OP_DIV_QUICK, u, nu, dt)
    ctx.rk_stage(phis[0], phi0[0], out[0], 0.75, 0.25, L.OP_DIV_QUICK, u, nu, dt)


def test_every_case_runs_on_the_kernel_it_is_meant_for():
    """the launch log (PYAPES_HIP_DEBUG=1) of one Euler step and one fused stage per case, in ONE child process"""
    code = ("import torch\nimport test_gpu_quick as T\n"
            "for name in T.NAMES:\n"
            "    torch.cuda.synchronize(); sys.stderr.write('CASE %s\\n' % name); sys.stderr.flush()\n"
            "    T._step_and_stage(name)\n"
            "    torch.cuda.synchronize(); sys.stderr.flush()\n")
    kernels = ("k_sfq", "k_euler", "k_sf ", "k_cg3d", "k_rk_combine")
    seen = G.case_log(G.child(code), lambda ln: "[pyapes_hip]" in ln and any(k in ln for k in kernels))
    for name, n, dtype, bcs, u, *_, kernel in CASES:
        lines = seen[name]
        assert not any("k_sf " in ln or "k_cg3d" in ln for ln in lines), (name, lines)   # the other tiled paths decline the kind
        sfq = [ln for ln in lines if "k_sfq " in ln]
        periodic = "periodic" in bcs[1]
        if kernel == "k_sfq":
            # (every k_sfq instantiation is launched fewer than eight times here: its log is not exhausted)
            assert len(sfq) == 2 and not any("k_euler" in ln for ln in lines), (name, lines)
            assert all("kind 5" in ln for ln in sfq), (name, lines)
            if periodic:   # the stage is the step kernel + the combine kernel
                assert not any("(RK stage)" in ln for ln in sfq) and any("k_rk_combine" in ln for ln in lines), (name, lines)
            else:
                assert sum("(RK stage)" in ln for ln in sfq) == 1, (name, lines)
            if u == "self":
                assert all("(self)" in ln and "(speed field)" in ln for ln in sfq), (name, lines)
            elif u == "field":
                assert all("(speed field)" in ln and "(self)" not in ln for ln in sfq), (name, lines)
            else:
                assert all(("(u >= 0)" if u >= 0 else "(u < 0)") in ln for ln in sfq), (name, lines)
        else:
            assert not sfq, (name, lines)
            if not periodic:   # (the generic Euler step itself has no log line; its fused stage has)
                assert any("k_euler (RK stage)" in ln for ln in lines), (name, lines)


# ---- 2. rows per wave -----------------------------------------------------------------------------------------------
# The dispatcher (csrc/pa_sf_kernel.h sf_variant) picks TWO rows per wave on every mesh unless option "sfq" is 4, and the
# option values 2 / 4 force a row count on any mesh -- so [40, 36, 72] (three tiles of 16 rows, the last one partly
# filled; six of 8 rows) is the smallest mesh that reaches both instantiations with more than one tile and an overhanging one.
def rows_per_wave_case():
    worst = {}
    for name in ("sfq_f32_config4", "sfq_f64_mixed", "sfq_f32_speed_field", "sfq_f64_allneu_uneg"):
        outs = {}
        for rows in (0, 2, 4):
            mesh, bc, phis, phi0, u, nu, dt = _setup(name)
            ctx = context_for(mesh)
            ctx.set_option("sfq", rows)
            f = G.fresh_field(mesh, bc, phis)
            ctx.bind_bcs(f(), f.bcs, 0)
            a, b = torch.full_like(phis, float("nan")), torch.full_like(phis, float("nan"))
            ctx.euler_step(phis[0], a[0], L.OP_DIV_QUICK, u, nu, dt)
            ctx.rk_stage(phis[0], phi0[0], b[0], 0.75, 0.25, L.OP_DIV_QUICK, u, nu, dt)
            outs[rows] = (a, b)
        for rows in (2, 4):
            worst[name, rows] = all(bool(torch.equal(p, q)) and bool(torch.isfinite(p).all()) for p, q in zip(outs[rows], outs[0]))
    return worst


def test_rows_per_wave():
    log = G.child("import torch\nimport test_gpu_quick as T\n"
                  "w = T.rows_per_wave_case(); torch.cuda.synchronize()\n"
                  "assert all(w.values()), w\n")
    lines = [ln for ln in log.splitlines() if "k_sfq " in ln]
    assert len(lines) == 16, log[-3000:]             # four cases x (two rows, four rows) x (step, stage)
    assert sum(" RJ 2 " in ln for ln in lines) == 8 and sum(" RJ 4 " in ln for ln in lines) == 8, lines


# ---- 3. the stage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_stage_is_the_composition_bit_for_bit(name):
    mesh, bc, phis, phi0, u, nu, dt = _setup(name)
    for c0, c1 in R.ALL4:
        a = R._fused(mesh, bc, QUICK, phis, phi0, c0, c1, u, nu, dt)
        b = R._composition(mesh, bc, QUICK, phis, phi0, c0, c1, u.clone() if isinstance(u, torch.Tensor) else u, nu, dt)
        assert bit_equal(a, b), (c0, c1, float((a - b).abs().max()), int((a != b).sum()))


# ---- 4. the march ---------------------------------------------------------------------------------------------------
MARCH_CASES = ["sfq_f32_config4", "sfq_f64_mixed", "sfq_f32_speed_field", "sfq_f64_yperiodic", "sfq_f64_short_chunks_uneg",
               "gen_f32_odd_rows", "gen_f64_2d", "gen_f64_1d"]


@pytest.mark.parametrize("name", MARCH_CASES)
@pytest.mark.parametrize("order", [1, 2, 3])
def test_march_is_its_stages(name, order):
    import test_gpu_self_march as S
    mesh, bc, phis, _, u, nu, dt = _setup(name)
    for nsteps in (1, 2, 3, 5):
        f = G.fresh_field(mesh, bc, phis, time=True)
        assert rk_march(f, u, nu, dt, nsteps, QUICK, order=order) is f
        ref = R._march_by_stages(mesh, bc, QUICK, phis, u, nu, dt, order, nsteps)
        assert bit_equal(f(), ref), (nsteps, float((f() - ref).abs().max()))
        assert abs(float(f.t) - (1.5 + nsteps * dt)) <= 1e-12
        if order == 1:
            assert bit_equal(euler_march(G.fresh_field(mesh, bc, phis), u, nu, dt, nsteps, QUICK)(), ref)
        # the field advects itself: every stage by its own input
        g = G.fresh_field(mesh, bc, phis, time=True)
        assert rk_march(g, g, nu, dt, nsteps, QUICK, order=order) is g
        sref = S._self_march_by_pieces(mesh, bc, QUICK, phis, nu, dt, order, nsteps)
        assert bit_equal(g(), sref), (nsteps, float((g() - sref).abs().max()))
        assert abs(float(g.t) - (1.5 + nsteps * dt)) <= 1e-12
    f = rk_step(G.fresh_field(mesh, bc, phis), u, nu, dt, QUICK, order=order)
    assert bit_equal(f(), R._march_by_stages(mesh, bc, QUICK, phis, u, nu, dt, order, 1))


def test_march_equals_the_restatement():
    """three order-3 steps, frozen speed and self-advected, against the CPU march of tests/march_ref.py"""
    for name in ("sfq_f64_mixed", "sfq_f32_config4"):
        mesh, bc, phis, _, u, nu, dt = _setup(name)
        om, ob = _oracle_side(name, mesh)
        a = rk_march(G.fresh_field(mesh, bc, phis), u, nu, dt, 3, QUICK, order=3)()
        assert bit_equal(a, Q.march(phis.cpu().clone(), u, nu, dt, 3, om, ob, "quick", 3))
        g = G.fresh_field(mesh, bc, phis)
        assert bit_equal(rk_march(g, g, nu, dt, 3, QUICK, order=3)(), Q.march(phis.cpu().clone(), None, nu, dt, 3, om, ob, "quick", 3, self_adv=True))


# ---- 5. switches ----------------------------------------------------------------------------------------------------
def _march_with(name, options, self_adv=False):
    mesh, bc, phis, _, u, nu, dt = _setup(name)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    f = G.fresh_field(mesh, bc, phis)
    rk_march(f, f if self_adv else u, nu, dt, 4, QUICK, order=3)
    return f().clone()


@pytest.mark.parametrize("name", ["sfq_f32_config4", "sfq_f64_allneu_uneg", "sfq_f64_mixed", "sfq_f32_speed_field", "sfq_f64_six_rows",
                                  "sfq_f64_yperiodic", "sfq_f32_two_ktiles"])
def test_switches_do_not_change_bits(name):
    for self_adv in (False, True):
        base = _march_with(name, {}, self_adv)
        for opt in ({"sfq": 0}, {"sfq": 2}, {"sfq": 4}, {"sf": 0}, {"fastpath": 0}, {"bcl": 0}, {"sfq": 1, "sf": 1, "fastpath": 1, "bcl": 1}):
            other = _march_with(name, opt, self_adv)
            assert bit_equal(base, other), (opt, self_adv, float((base - other).abs().max()))


@pytest.mark.parametrize("shape,dtype,bcs", [([40, 36, 72], "single", R.NEUSYM), ([21, 19, 34], "double", R.ALLDIR)])
def test_the_option_touches_nothing_else(shape, dtype, bcs):
    """the other three Div kinds: a 3-step order-3 march and the explicit Div give the same bits with "sfq" 0 and 1.
    (Central Div is refused on neumann / symmetry faces by every entry point, as in the reference: that kind runs with
    all-Dirichlet faces on both meshes.)"""
    for config in (R.UPWIND, R.COMPAT, R.CENTRAL):
        outs = []
        for sfq in (1, 0):
            mesh = Mesh(Box[0:1, 0:1, 0:1], None, shape, "cuda", dtype)
            context_for(mesh).set_option("sfq", sfq)
            bc = {"domain": mixed_bcs(*(R.ALLDIR if config is R.CENTRAL else bcs)), "obstacle": None}
            g = torch.Generator().manual_seed(3)
            f = Field("phi", 1, mesh, bc)
            f.set_var_tensor(torch.rand((1, *shape), generator=g, dtype=torch.float64).to(mesh.dtype.float).cuda())
            f.apply_bcs()
            d = FDC(config).div(0.7, f).clone()
            dx = min(float(h) for h in mesh.dx_list)
            rk_march(f, 0.7, 1e-3, 0.1 * dx, 3, config, order=3)
            outs.append((d, f().clone()))
        assert bit_equal(outs[0][0], outs[1][0]) and bit_equal(outs[0][1], outs[1][1]), config


# ---- 6. the CPU facts of tests/test_quick_host.py, through rk_march -------------------------------------------------
def _line_field(n, hi, start):
    mesh = Mesh(Box[0:hi], None, [n], "cuda", "double")
    bc = {"domain": mixed_bcs([0.0, 0.0], ["dirichlet", "dirichlet"]), "obstacle": None}
    f = Field("phi", 1, mesh, bc)
    f.set_var_tensor(start.cuda())
    f.apply_bcs()
    return f


def test_mirror_symmetry_on_the_gpu():
    om, ob = H._line(201)
    g = H._gauss(om, ob, 0.6)
    dt = 0.4 * om.dx_list[0]
    a = rk_march(_line_field(201, 2, g), 1.0, 0.0, dt, 50, QUICK, order=3)()
    b = rk_march(_line_field(201, 2, torch.flip(g, [1]).contiguous()), -1.0, 0.0, dt, 50, QUICK, order=3)()
    assert bit_equal(a, torch.flip(b, [1]))
    assert float((a.cpu() - g).abs().max()) > 0.1


def test_stability_on_the_gpu():
    start = H.stability_start()
    dx = 1.0 / 128
    euler = float(rk_march(_line_field(129, 1, start), 1.0, 0.0, 0.5 * dx, 600, QUICK, order=1)().abs().max())
    rk3 = float(rk_march(_line_field(129, 1, start), 1.0, 0.0, 1.0 * dx, 600, QUICK, order=3)().abs().max())
    print(f"stability on the GPU: Euler CFL 0.5 -> {euler:.3e}, order 3 CFL 1.0 -> {rk3:.3e}")
    assert euler > 1e6
    assert rk3 <= 1.0


@pytest.mark.parametrize("self_adv", [False, True], ids=["u=1", "self"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_order_in_time_on_the_gpu(order, self_adv):
    mesh, bc, phi0 = R._pulse_case()
    nu, T = 0.05, 0.02

    def march(n, o):
        f = G.fresh_field(mesh, bc, phi0)
        return rk_march(f, f if self_adv else 1.0, nu, T / n, n, QUICK, order=o)().clone()

    ref = march(640, 3)
    err = [float((march(n, order) - ref).abs().max()) for n in (20, 40, 80)]
    ratios = (err[0] / err[1], err[1] / err[2])
    print(f"order {order} self {self_adv}: errors {err}, ratios {ratios}")
    lo, hi = H.ORDER_BOUNDS[order]
    for r in ratios:
        assert lo < r < hi, (order, self_adv, err, ratios)


def test_burgers_on_the_gpu():
    import math

    def march(start, ends, dt, steps):
        n = start.shape[1]
        mesh = Mesh(Box[0:2 * math.pi], None, [n], "cuda", "double")
        bc = {"domain": mixed_bcs(list(ends), ["dirichlet", "dirichlet"]), "obstacle": None}
        f = Field("phi", 1, mesh, bc)
        f.set_var_tensor(start.cuda())
        f.apply_bcs()
        return rk_march(f, f, HS.BURGERS_NU, dt, steps, QUICK, order=3)()
    H.check_burgers(*(HS.burgers_error(n, "quick", march) for n in (101, 201)))


# ---- 7. errors ------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    mesh, bc, phis, phi0, u, nu, dt = _setup("sfq_f64_mixed")
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, phis)
    # an axis of 4 nodes: PA_E_ARG from every entry point that takes the kind
    small = Mesh(Box[0:1, 0:1, 0:1], None, [16, 4, 32], "cuda", "double")
    sbc = {"domain": mixed_bcs(*R.MIXED), "obstacle": None}
    sf = Field("phi", 1, small, sbc)
    sf.set_var_tensor(torch.rand((1, 16, 4, 32), dtype=torch.float64, device="cuda"))
    with pytest.raises(PaError, match="5 nodes"):
        FDC(QUICK).div(1.0, sf)
    with pytest.raises(PaError, match="5 nodes"):
        euler_step(sf, 1.0, nu, dt, QUICK)
    with pytest.raises(PaError, match="5 nodes"):
        euler_march(sf, 1.0, nu, dt, 2, QUICK)
    with pytest.raises(PaError, match="5 nodes"):
        rk_march(sf, sf, nu, dt, 2, QUICK, order=3)
    with pytest.raises(PaError, match="5 nodes"):
        rk_march(sf, 1.0, nu, dt, 2, QUICK, order=3)
    # a slab context at the C ABI: PA_E_STATE with a message
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    sctx = context_for(slab)
    sphi = torch.zeros(tuple(slab.nx), dtype=torch.float64, device="cuda")
    w1, w2 = torch.empty_like(sphi), torch.empty_like(sphi)
    with pytest.raises(PaError, match="single GPU"):
        sctx.euler_step(sphi, w1, L.OP_DIV_QUICK, 1.0, nu, dt)
    with pytest.raises(PaError, match="single GPU"):
        sctx.div(L.OP_DIV_QUICK, 1.0, sphi, out=w1)
    with pytest.raises(PaError, match="single GPU"):
        sctx.rk_march(sphi, w1, w2, 3, L.OP_DIV_QUICK, 1.0, nu, dt, 2)
    with pytest.raises(PaError, match="single GPU"):
        sctx.rk_march_self(sphi, w1, w2, 3, L.OP_DIV_QUICK, nu, dt, 2)
    slab_field = Field("phi", 1, slab, {"domain": mixed_bcs(*R.MIXED), "obstacle": None})
    with pytest.raises(NotImplementedError):
        rk_march(slab_field, 1.0, nu, dt, 2, QUICK)
    # an axisymmetric mesh: refused in Python and at the C ABI
    cyl = Mesh(Cylinder[0:1, 0:1], None, [16, 16], "cuda", "double")
    cctx = context_for(cyl)
    cphi = torch.zeros((16, 16), dtype=torch.float64, device="cuda")
    with pytest.raises(PaError, match="xyz"):
        cctx.div(L.OP_DIV_QUICK, 1.0, cphi, out=torch.empty_like(cphi))
    with pytest.raises(PaError, match="xyz"):
        cctx.euler_step(cphi, torch.empty_like(cphi), L.OP_DIV_QUICK, 1.0, nu, dt)
    # solver equations: pa_eq_set refuses the kind
    ctx.bind_bcs(f(), f.bcs, 0)
    with pytest.raises(PaError, match="explicit-only"):
        ctx.set_terms([{"kind": L.OP_DIV_QUICK, "sign": 1.0, "u": 1.0}])
    with pytest.raises(PaError):
        ctx.div_general(L.OP_DIV_QUICK, False, [phis[0]] * 3, 1.0, [None] * 3, [None] * 3, torch.empty_like(phis[0]))
    # the context that saw the errors still marches, and gives what a fresh one gives
    a = rk_march(G.fresh_field(mesh, bc, phis), u, nu, dt, 2, QUICK)().clone()
    mesh_b, bc_b, phis_b, _, _, _, _ = _setup("sfq_f64_mixed")
    b = rk_march(G.fresh_field(mesh_b, bc_b, phis_b), u, nu, dt, 2, QUICK)()
    assert bit_equal(phis, phis_b) and bit_equal(a, b)
