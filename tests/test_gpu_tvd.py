"""-m gpu: the slope-limited (TVD) advection schemes, Div limiters "minmod" and "mc" (PA_OP_DIV_MINMOD / PA_OP_DIV_MC: the
generic kernels through pa_tvd_halves of csrc/pa_device.h, the SCH instantiations of the marching kernel k_sfq in
csrc/pa_sft.hip).

The yardstick of the BITS is tests/march_ref.py, the torch-CPU restatement of the definition: FDC.div at every node, the Euler
step and two fused Runge-Kutta stages must equal it bit for bit, fp32 and fp64, both limiters, on k_sfq and on the generic
kernel (option "sfq" 0 included), on the small meshes tests/test_gpu_quick.py uses because they are the smallest that reach
each code path.  The fields mix random values with values on a grid of quarters, so that flat runs (differences that are
exact zeros), slope sign changes and both same-sign branches of minmod occur in every row block -- asserted on the CPU side.
The launch log shows which kernel ran; the marches must be their stages and equal the restated marches; the bounded block of
tests/test_tvd_host.py must stay inside [0, 1] exactly on the GPU.
"""
import sys

import pytest
import torch

import march_gpu as G
import march_ref as Q
import pyapes_oracle as O
import test_gpu_rk as R
import test_tvd_host as H
from helpers import bit_equal, offset_view
from march_gpu import XPER
from pyapes_amd.geometry import Box, Cylinder
from pyapes_amd.hip import lib as L
from pyapes_amd.hip.context import context_for
from pyapes_amd.hip.lib import PaError
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import FDC
from pyapes_amd.solver.march import euler_march, euler_step, momentum_march, rk_march, rk_step
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

LIMITERS = ("minmod", "mc")
CONFIG = H.CONFIG
KIND = {"minmod": L.OP_DIV_MINMOD, "mc": L.OP_DIV_MC}
STAGES = [(0.75, 0.25), (1.0 / 3.0, 2.0 / 3.0)]

# name, n, dtype, bcs, u ("field": a randn speed tensor, "self": the field itself), operands misaligned, context options,
# the kernel the Euler step must run on
CASES = [
    ("sft_f64_mixed", [21, 19, 34], "double", R.MIXED, 0.6, False, {}, "k_sfq"),                   # fallback rows, odd row count
    ("sft_f64_allneu_uneg", [24, 20, 66], "double", R.ALLNEU, -0.8, False, {}, "k_sfq"),           # the other US half
    ("sft_f32_speed_field", [20, 24, 64], "single", R.NEUSYM, "field", False, {}, "k_sfq"),        # both signs in one row
    ("sft_f64_two_ktiles_field", [12, 20, 136], "double", R.ALLDIR, "field", False, {}, "k_sfq"),  # the edge-cell pairs
    ("sft_f32_two_ktiles", [9, 40, 264], "single", R.ALLDIR, 1.3, False, {}, "k_sfq"),             # several row tiles, two k tiles
    ("sft_f64_yperiodic", [16, 20, 40], "double", R.YPER, -1.1, False, {}, "k_sfq"),               # (stage: + k_rk_combine)
    ("sft_f64_self", [21, 19, 34], "double", R.MIXED, "self", False, {}, "k_sfq"),
    ("sft_f32_sfq4_is_two_rows", [20, 24, 64], "single", R.NEUSYM, 0.7, False, {"sfq": 4}, "k_sfq"),
    ("gen_f64_xperiodic", [16, 20, 40], "double", XPER, 0.7, False, {}, "k_euler"),
    ("gen_f64_2d", [33, 48], "double", R.MIX2D, -0.7, False, {}, "k_euler"),
    ("gen_f64_1d", [65], "double", R.MIX1D, 0.8, False, {}, "k_euler"),
    ("gen_f32_odd_rows", [17, 19, 33], "single", R.MIXED, 0.9, False, {}, "k_euler"),
    ("gen_f32_misaligned", [20, 24, 64], "single", R.NEUSYM, 1.0, True, {}, "k_euler"),
    ("gen_f32_sfq_off", [20, 24, 64], "single", R.NEUSYM, "field", False, {"sfq": 0}, "k_euler"),
]
CASE = {c[0]: c for c in CASES}
NAMES = [c[0] for c in CASES]
SFT_NAMES = [c[0] for c in CASES if c[-1] == "k_sfq"]


def mixed_data(shape, g, tdt):
    """random values, about half of them moved onto the grid of quarters: flat runs, sign changes of the slope, exact zeros"""
    raw = torch.rand(shape, generator=g, dtype=torch.float64)
    grid = torch.round(4.0 * torch.rand(shape, generator=g, dtype=torch.float64)) / 4.0
    pick = torch.rand(shape, generator=g, dtype=torch.float64) < 0.5
    return torch.where(pick, grid, raw).to(tdt)


def branches_in_every_row_block(x):
    """on the CPU: along every mesh axis, in every block of 8 rows (all rows of a 1-D / 2-D field) of every plane, the pairs
    (dm, dp) hit the three branches of minmod1 -- both >= 0 with a positive result, both < 0, and a * b <= 0 -- the last one
    both as an exact zero (a flat run) and as a sign change of the slope.  (3-D: the planes 2 .. n0 - 3.  The two planes at an
    axis-0 face hold what the BC fill leaves there -- a constant dirichlet plane, a neumann plane whose slope along axis 0 has
    the sign of the one behind it -- so no data can put every branch there.)"""
    nd = x.dim()
    for a in range(nd):
        dm = x - torch.roll(x, 1, a)
        dp = torch.roll(x, -1, a) - x
        facts = [(dm > 0) & (dp > 0), (dm < 0) & (dp < 0), (dm * dp) == 0, (dm * dp) < 0]
        for f in facts:
            if nd == 3:
                f = f[2:-2]
            f3 = f.reshape((-1,) + tuple(f.shape[-2:])) if nd >= 2 else f.reshape(1, 1, -1)
            for j0 in range(0, f3.shape[1], 8):
                blk = f3[:, j0:j0 + 8, :]
                if blk.shape[1] * blk.shape[2] >= 64 and not bool(blk.reshape(blk.shape[0], -1).any(1).all()):
                    return False
    return True


_SETUPS = {}


def _setup(name, seed=17):
    """mesh, BC config, oracle mesh and BCs, (phi_s, phi0) BC-filled on the device, the speed (device), nu, dt.  A misaligned
    case hands out phi_s as a contiguous view one element into a larger allocation."""
    _, n, dtype, bcs, u, misaligned, options, _ = CASE[name]
    nd = len(n)
    mesh = Mesh(G.box(nd), None, n, "cuda", dtype)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    if name not in _SETUPS:
        om = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
        ob = O.make_bcs(om, O.mixed_cfg(list(bcs[0]), list(bcs[1]), O.FACES[:2 * nd]))
        g = torch.Generator().manual_seed(seed)
        tdt = mesh.dtype.float
        fields = [O.bc_fill(mixed_data((1, *n), g, tdt), ob) for _ in range(2)]
        assert branches_in_every_row_block(fields[0][0]), name
        speed = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        _SETUPS[name] = (om, ob, fields[0], fields[1], speed)
    om, ob, phis_c, phi0_c, speed = _SETUPS[name]
    bc = {"domain": mixed_bcs(*bcs), "obstacle": None}
    phis, phi0 = phis_c.cuda(), phi0_c.cuda()
    if misaligned:
        phis, _ = offset_view(phis, 1)
        assert phis.is_contiguous() and phis.data_ptr() % 16 != 0 and torch.equal(phis.cpu(), phis_c)
    uu = phis if u == "self" else (speed.cuda() if u == "field" else u)
    dx = min(float(d) for d in mesh.dx_list)
    nu = 1e-3
    dt = 0.2 * min(dx * dx / (2 * nd * nu), dx / 1.3)
    return mesh, bc, om, ob, phis, phi0, uu, nu, dt


def _ref_speed(u):
    return u.cpu().clone() if isinstance(u, torch.Tensor) else u


# ---- 1. bits against the restatement --------------------------------------------------------------------------------
def _device_results(name, lim, sfq=None):
    """(div, euler step, the two stages) of the case on the device; sfq: option "sfq" for this context"""
    mesh, bc, om, ob, phis, phi0, u, nu, dt = _setup(name)
    ctx = context_for(mesh)
    if sfq is not None:
        ctx.set_option("sfq", sfq)
    f = G.fresh_field(mesh, bc, phis)
    if phis.data_ptr() % 16 != 0:
        f.set_var_tensor(phis)                       # keep the misaligned storage
    outs = [FDC(CONFIG[lim]).div(u.clone() if isinstance(u, torch.Tensor) else u, f).clone()]
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.full_like(phi0, float("nan"))
    ctx.euler_step(phis[0], out[0], KIND[lim], u, nu, dt)          # (u is phis itself in the self cases)
    outs.append(out)
    for c0, c1 in STAGES:
        out = torch.full_like(phi0, float("nan"))
        ctx.rk_stage(phis[0], phi0[0], out[0], c0, c1, KIND[lim], u, nu, dt)
        outs.append(out)
    return outs


@pytest.mark.parametrize("lim", LIMITERS)
@pytest.mark.parametrize("name", NAMES)
def test_div_step_and_stages_are_the_restatement_bit_for_bit(name, lim):
    mesh, bc, om, ob, phis, phi0, u, nu, dt = _setup(name)
    x, x0 = phis.cpu().clone(), phi0.cpu().clone()
    uc = x if CASE[name][4] == "self" else _ref_speed(u)
    refs = [Q.div_tvd(uc, x, om, ob, lim), Q.euler_step(x, uc, nu, dt, om, ob, lim)]
    refs += [Q.rk_stage(x, x0, c0, c1, uc, nu, dt, om, ob, lim) for c0, c1 in STAGES]
    assert all(bool(torch.isfinite(r).all()) for r in refs)
    got = _device_results(name, lim)
    for what, a, b in zip(("div", "euler_step", "stage 3/4 1/4", "stage 1/3 2/3"), got, refs):
        assert bit_equal(a, b), (what, float((a.cpu() - b).abs().max()), int((a.cpu() != b).sum()))
    if name in SFT_NAMES:   # tiled against the generic kernel
        for what, a, b in zip(("div", "euler_step", "stage", "stage"), got, _device_results(name, lim, sfq=0)):
            assert bit_equal(a, b), ("sfq 0", what)
    g = euler_step(G.fresh_field(mesh, bc, phis), u if CASE[name][4] != "self" else phis.clone(), nu, dt, CONFIG[lim])   # the public entry
    assert bit_equal(g(), refs[1])


@pytest.mark.parametrize("lim", LIMITERS)
@pytest.mark.parametrize("u", [0.9, -0.9, "field"], ids=["upos", "uneg", "field"])
def test_chunks_of_every_length(u, lim):
    """[13, 12, 32] under option "chunks" 1, 2, 3, 5: chunk lengths 13 | 6, 7 | 4, 4, 5 | 2, 2, 3, 3, 3 -- every remainder of the
    plane loop's unroll by six, and one chunk that holds both axis-0 faces"""
    n, bcs = [13, 12, 32], R.MIXED
    om = O.OMesh([0.0] * 3, [1.0] * 3, n, "double")
    ob = O.make_bcs(om, O.mixed_cfg(list(bcs[0]), list(bcs[1]), O.FACES))
    g = torch.Generator().manual_seed(23)
    x, x0 = (O.bc_fill(mixed_data((1, *n), g, torch.float64), ob) for _ in range(2))
    assert branches_in_every_row_block(x[0])
    uc = torch.randn((1, *n), generator=g, dtype=torch.float64) if u == "field" else u
    nu, dt = 1e-3, 0.2 * (1.0 / 31) / 1.3
    refs = [Q.euler_step(x, uc, nu, dt, om, ob, lim), Q.rk_stage(x, x0, 0.75, 0.25, uc, nu, dt, om, ob, lim)]
    for chunks in (1, 2, 3, 5):
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, n, "cuda", "double")
        ctx = context_for(mesh)
        ctx.set_option("chunks", chunks)
        f = G.fresh_field(mesh, {"domain": mixed_bcs(*bcs), "obstacle": None}, x)
        ctx.bind_bcs(f(), f.bcs, 0)
        ud = uc.cuda() if u == "field" else u
        a, b = torch.full_like(f(), float("nan")), torch.full_like(f(), float("nan"))
        ctx.euler_step(f()[0], a[0], KIND[lim], ud, nu, dt)
        ctx.rk_stage(f()[0], x0.cuda()[0], b[0], 0.75, 0.25, KIND[lim], ud, nu, dt)
        ctx.set_option("chunks", 0)
        assert bit_equal(a, refs[0]) and bit_equal(b, refs[1]), chunks


# ---- 2. routing -----------------------------------------------------------------------------------------------------
def _step_and_stage(name, lim):
    mesh, bc, om, ob, phis, phi0, u, nu, dt = _setup(name)
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, phis)
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.empty_like(phi0)
    ctx.euler_step(phis[0], out[0], KIND[lim], u, nu, dt)
    ctx.rk_stage(phis[0], phi0[0], out[0], 0.75, 0.25, KIND[lim], u, nu, dt)


def _source_and_velocity(lim):
    """on a mesh k_sfq takes: the step and the stage with a source, then in a velocity"""
    mesh, bc, om, ob, phis, phi0, u, nu, dt = _setup("sft_f64_mixed")
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, phis)
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.empty_like(phi0)
    sys.stderr.write("CASE source\n"); sys.stderr.flush()
    ctx.euler_step(phis[0], out[0], KIND[lim], u, nu, dt, source=0.5)
    ctx.rk_stage(phis[0], phi0[0], out[0], 0.75, 0.25, KIND[lim], u, nu, dt, source=0.5)
    torch.cuda.synchronize(); sys.stderr.write("CASE velocity\n"); sys.stderr.flush()
    ctx.euler_step_vel(phis[0], out[0], KIND[lim], [0.5, -0.25, 1.0], nu, dt)
    ctx.rk_stage_vel(phis[0], phi0[0], out[0], 0.75, 0.25, KIND[lim], [0.5, -0.25, 1.0], nu, dt)
    torch.cuda.synchronize()


@pytest.mark.parametrize("lim", LIMITERS)
def test_every_case_runs_on_the_kernel_it_is_meant_for(lim):
    """the launch log (PYAPES_HIP_DEBUG=1) of one Euler step and one fused stage per case, in ONE child process per limiter"""
    code = ("import torch\nimport test_gpu_tvd as T\n"
            "for name in T.NAMES:\n"
            "    torch.cuda.synchronize(); sys.stderr.write('CASE %s\\n' % name); sys.stderr.flush()\n"
            f"    T._step_and_stage(name, {lim!r})\n"
            "    torch.cuda.synchronize(); sys.stderr.flush()\n"
            f"T._source_and_velocity({lim!r})\n")
    kernels = ("k_sfq", "k_euler", "k_sf ", "k_cg3d", "k_rk_combine")
    seen = G.case_log(G.child(code), lambda ln: "[pyapes_hip]" in ln and any(k in ln for k in kernels))
    for name, n, dtype, bcs, u, *_, kernel in CASES:
        lines = seen[name]
        assert not any("k_sf " in ln or "k_cg3d" in ln for ln in lines), (name, lines)   # the other tiled paths decline the kind
        sfq = [ln for ln in lines if "k_sfq " in ln]
        periodic = "periodic" in bcs[1]
        if kernel == "k_sfq":
            assert len(sfq) == 2 and not any("k_euler" in ln for ln in lines), (name, lines)
            assert all(f"kind {KIND[lim]} RJ 2" in ln for ln in sfq), (name, lines)
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
    for case, tag in (("source", "(source): generic kernel"), ("velocity", "(velocity): generic kernel")):
        lines = seen[case]
        assert not any("k_sfq" in ln or "k_sf " in ln or "k_cg3d" in ln for ln in lines), (case, lines)
        assert sum(tag in ln for ln in lines) == 2 and sum("(RK stage)" in ln for ln in lines) == 1, (case, lines)


@pytest.mark.parametrize("lim", LIMITERS)
def test_source_and_velocity_are_the_restatement(lim):
    """(the generic kernel) a source field and a scalar source, a velocity of numbers and of fields, step and stage"""
    mesh, bc, om, obcs, phi_c, phi0_c, speed, src_c, nu, dt = G.setup([21, 19, 34], "double", "mix", 3)
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, phi_c)
    ctx.bind_bcs(f(), f.bcs, 0)
    phi_d, phi0_d = phi_c.cuda(), phi0_c.cuda()
    one = speed[:1]
    for s_ref, s_dev in ((src_c, src_c.cuda()[0]), (0.75, 0.75)):
        out = torch.full_like(phi_d, float("nan"))
        ctx.euler_step(phi_d[0], out[0], KIND[lim], one.cuda(), nu, dt, source=s_dev)
        assert bit_equal(out, Q.euler_step(phi_c, one, nu, dt, om, obcs, lim, s_ref))
        out = torch.full_like(phi_d, float("nan"))
        ctx.rk_stage(phi_d[0], phi0_d[0], out[0], 0.75, 0.25, KIND[lim], -0.7, nu, dt, source=s_dev)
        assert bit_equal(out, Q.rk_stage(phi_c, phi0_c, 0.75, 0.25, -0.7, nu, dt, om, obcs, lim, s_ref))
    for v_ref, v_dev in (([0.5, -0.25, 1.0],) * 2, ([speed[a] for a in range(3)], [speed[a].cuda() for a in range(3)])):
        out = torch.full_like(phi_d, float("nan"))
        ctx.euler_step_vel(phi_d[0], out[0], KIND[lim], v_dev, nu, dt)
        assert bit_equal(out, Q.euler_step(phi_c, v_ref, nu, dt, om, obcs, lim))
        out = torch.full_like(phi_d, float("nan"))
        ctx.rk_stage_vel(phi_d[0], phi0_d[0], out[0], 1.0 / 3.0, 2.0 / 3.0, KIND[lim], v_dev, nu, dt, source=src_c.cuda()[0])
        assert bit_equal(out, Q.rk_stage(phi_c, phi0_c, 1.0 / 3.0, 2.0 / 3.0, v_ref, nu, dt, om, obcs, lim, src_c))


# ---- 3. the marches -------------------------------------------------------------------------------------------------
MARCH_CASES = ["sft_f64_mixed", "sft_f32_speed_field", "sft_f64_yperiodic", "gen_f32_odd_rows", "gen_f64_2d"]


@pytest.mark.parametrize("lim", LIMITERS)
@pytest.mark.parametrize("name", MARCH_CASES)
@pytest.mark.parametrize("order", [1, 2, 3])
def test_march_is_its_stages(name, order, lim):
    mesh, bc, om, ob, phis, _, u, nu, dt = _setup(name)
    cfg = CONFIG[lim]
    for nsteps in (1, 3):
        f = G.fresh_field(mesh, bc, phis, time=True)
        assert rk_march(f, u, nu, dt, nsteps, cfg, order=order) is f
        ref = R._march_by_stages(mesh, bc, cfg, phis, u, nu, dt, order, nsteps)
        assert bit_equal(f(), ref), (nsteps, float((f() - ref).abs().max()))
        assert abs(float(f.t) - (1.5 + nsteps * dt)) <= 1e-12
        if order == 1:
            assert bit_equal(euler_march(G.fresh_field(mesh, bc, phis), u, nu, dt, nsteps, cfg)(), ref)
    assert bit_equal(rk_step(G.fresh_field(mesh, bc, phis), u, nu, dt, cfg, order=order)(),
                     R._march_by_stages(mesh, bc, cfg, phis, u, nu, dt, order, 1))


@pytest.mark.parametrize("lim", LIMITERS)
def test_marches_equal_the_restatement(lim):
    """three order-3 steps with a frozen speed and self-advected, two in a velocity, and the momentum march"""
    cfg = CONFIG[lim]
    for name in ("sft_f64_mixed", "sft_f32_speed_field"):
        mesh, bc, om, ob, phis, _, u, nu, dt = _setup(name)
        x = phis.cpu().clone()
        a = rk_march(G.fresh_field(mesh, bc, phis), u, nu, dt, 3, cfg, order=3)()
        assert bit_equal(a, Q.march(x, _ref_speed(u), nu, dt, 3, om, ob, lim, 3)), name
        g = G.fresh_field(mesh, bc, phis)
        assert bit_equal(rk_march(g, g, nu, dt, 3, cfg, order=3)(), Q.march(x, None, nu, dt, 3, om, ob, lim, 3, self_adv=True)), name
    mesh, bc, om, obcs, phi_c, _, speed, src_c, nu, dt = G.setup([21, 19, 34], "double", "mix", 3)
    vel_c = [speed[a] for a in range(3)]
    for order in (1, 3):
        got = rk_march(G.fresh_field(mesh, bc, phi_c), [v.cuda() for v in vel_c], nu, dt, 2, cfg, order=order)()
        assert bit_equal(got, Q.march(phi_c, vel_c, nu, dt, 2, om, obcs, lim, order)), order
    import test_gpu_momentum as GM
    for n, dtype in (([9, 14, 132], "double"), ([17, 12], "double")):
        mesh, bc, om, obcs, _, U_c, src_c, _, nu, dt = GM._setup(n, dtype, "mix")
        got = momentum_march(G.fresh_field(mesh, bc, U_c), nu, dt, 2, cfg, order=3)()
        assert bit_equal(got, Q.momentum.march(U_c, nu, dt, 2, om, obcs, lim, 3)), n
        srcs = [src_c[c] for c in range(len(n))]
        got = momentum_march(G.fresh_field(mesh, bc, U_c), nu, dt, 1, cfg, order=2, source=[s.cuda() for s in srcs])()
        assert bit_equal(got, Q.momentum.march(U_c, nu, dt, 1, om, obcs, lim, 2, srcs)), n


@pytest.mark.parametrize("lim", LIMITERS)
def test_the_bounded_block_stays_inside_its_bounds(lim):
    """the 12 x 14 x 16 block of tests/test_tvd_host.py, 40 order-3 steps on k_sfq: one speed of each sign and a speed field
    with both signs; 0 <= phi <= 1 exactly, and the bits of the restatement"""
    om, ob, phi, _, _ = H.block_case("double")
    mesh = Mesh(Box[0:1, 0:1, 0:1], None, [12, 14, 16], "cuda", "double")
    bc = {"domain": mixed_bcs([0.0] * 6, ["dirichlet"] * 6), "obstacle": None}
    x, y, z = om.grid
    field = (torch.cos(3.0 * x) * torch.cos(5.0 * y + 2.0 * z)).unsqueeze(0).contiguous()
    assert float(field.min()) < -0.5 and float(field.max()) > 0.5 and float(field.abs().max()) <= 1.0
    dt = 0.45 / sum(1.0 / h for h in om.dx_list)          # |u| <= 1 on every axis
    for u in (1.0, -1.0, field):
        got = rk_march(G.fresh_field(mesh, bc, phi), u.cuda() if isinstance(u, torch.Tensor) else u, 0.0, dt, 40, CONFIG[lim], order=3)()
        lo, hi = float(got.min()), float(got.max())
        print(f"block on the GPU, {lim}, u {'field' if isinstance(u, torch.Tensor) else u}: min {lo:.3e}, max - 1 {hi - 1:.3e}")
        assert lo >= 0.0 and hi <= 1.0, (lo, hi)
        assert float((got.cpu() - phi).abs().max()) > 0.3
        assert bit_equal(got, Q.march(phi, u, 0.0, dt, 40, om, ob, lim, 3))


# ---- 4. errors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lim", LIMITERS)
def test_errors_leave_the_context_usable(lim):
    cfg, kind = CONFIG[lim], KIND[lim]
    mesh, bc, om, ob, phis, phi0, u, nu, dt = _setup("sft_f64_mixed")
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, phis)
    # an axis of 4 nodes: PA_E_ARG from every entry point that takes the kind
    small = Mesh(Box[0:1, 0:1, 0:1], None, [16, 4, 32], "cuda", "double")
    sf = Field("phi", 1, small, {"domain": mixed_bcs(*R.MIXED), "obstacle": None})
    sf.set_var_tensor(torch.rand((1, 16, 4, 32), dtype=torch.float64, device="cuda"))
    for call in (lambda: FDC(cfg).div(1.0, sf), lambda: euler_step(sf, 1.0, nu, dt, cfg), lambda: euler_march(sf, 1.0, nu, dt, 2, cfg),
                 lambda: rk_march(sf, sf, nu, dt, 2, cfg, order=3), lambda: rk_march(sf, 1.0, nu, dt, 2, cfg, order=3),
                 lambda: rk_march(sf, (1.0, 1.0, 1.0), nu, dt, 2, cfg, order=3)):
        with pytest.raises(PaError, match=f"Div {lim} needs at least 5 nodes") as e:
            call()
        assert e.value.code == L.PA_E_ARG
    # a slab context at the C ABI: PA_E_STATE with a message
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    sctx = context_for(slab)
    sphi = torch.zeros(tuple(slab.nx), dtype=torch.float64, device="cuda")
    w1, w2 = torch.empty_like(sphi), torch.empty_like(sphi)
    for call in (lambda: sctx.euler_step(sphi, w1, kind, 1.0, nu, dt), lambda: sctx.div(kind, 1.0, sphi, out=w1),
                 lambda: sctx.rk_march(sphi, w1, w2, 3, kind, 1.0, nu, dt, 2), lambda: sctx.rk_march_self(sphi, w1, w2, 3, kind, nu, dt, 2)):
        with pytest.raises(PaError, match="single GPU") as e:
            call()
        assert e.value.code == L.PA_E_STATE
    # an axisymmetric mesh: refused at the C ABI
    cyl = Mesh(Cylinder[0:1, 0:1], None, [16, 16], "cuda", "double")
    cctx = context_for(cyl)
    cphi = torch.zeros((16, 16), dtype=torch.float64, device="cuda")
    for call in (lambda: cctx.div(kind, 1.0, cphi, out=torch.empty_like(cphi)),
                 lambda: cctx.euler_step(cphi, torch.empty_like(cphi), kind, 1.0, nu, dt)):
        with pytest.raises(PaError, match="xyz") as e:
            call()
        assert e.value.code == L.PA_E_ARG
    # solver equations: pa_eq_set refuses the kind, so pa_rhs_adjust finds no equation; pa_div_general refuses it
    ctx.bind_bcs(f(), f.bcs, 0)
    with pytest.raises(PaError, match="explicit-only") as e:
        ctx.set_terms([{"kind": kind, "sign": 1.0, "u": 1.0}])
    assert e.value.code == L.PA_E_ARG
    with pytest.raises(PaError):
        ctx.rhs_adjust(torch.zeros_like(phis[0]))
    with pytest.raises(PaError, match="explicit-only") as e:
        ctx.div_general(kind, False, [phis[0]] * 3, 1.0, [None] * 3, [None] * 3, torch.empty_like(phis[0]))
    assert e.value.code == L.PA_E_ARG
    with pytest.raises(PaError, match="bad div kind"):
        ctx.div(99, 1.0, phis[0], out=torch.empty_like(phis[0]))
    # the context that saw the errors still marches, and gives what a fresh one gives
    a = rk_march(G.fresh_field(mesh, bc, phis), u, nu, dt, 2, cfg)().clone()
    mesh_b, bc_b, _, _, phis_b, _, _, _, _ = _setup("sft_f64_mixed")
    b = rk_march(G.fresh_field(mesh_b, bc_b, phis_b), u, nu, dt, 2, cfg)()
    assert bit_equal(phis, phis_b) and bit_equal(a, b)
