"""-m gpu: the self-advected march, div(phi, phi) in the Euler and Runge-Kutta steps (pa_rk_march_self; the SELF
instantiations of k_sf, csrc/pa_sf_kernel.h / pa_sf_self.hip).

Handing a step its own input as the speed field -- u_field == phi_in at the C ABI -- has always been legal; it now runs on
kernels that read no speed stream and take the speed at the cell and at its neighbours from the stencil's operands.  The
yardstick of a single launch is therefore the same call with a CLONE of the field as the speed (the kernels with a speed
stream / the generic kernel): the BITS must be equal, on every kernel path.  The yardstick of the march is the loop of
public pieces that exist without the feature:
    phi0 = phi.clone();  cur = euler_step(Field(phi0), phi0.clone());  for (c0, c1): rk_stage(cur, phi0, out, u = cur.clone())
i.e. every stage advected by its own input -- which no march entry could express before (rk_march(f, f) kept one speed
pointer for the whole call).  The facts tests/test_self_march_host.py establishes on the CPU (order in time, Burgers'
equation) must hold through rk_march on the GPU with the same bounds.
"""
import math

import pytest
import torch

import march_gpu as G
import test_gpu_rk as R
import test_self_march_host as H
from helpers import bit_equal
from pyapes_amd.geometry import Box
from pyapes_amd.hip.context import context_for
from pyapes_amd.hip.lib import PaError
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import div_kind
from pyapes_amd.solver.march import euler_march, euler_step, rk_march, rk_step
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

UPWIND, COMPAT, CENTRAL = R.UPWIND, R.COMPAT, R.CENTRAL

# name, n, dtype, bcs, config, phi0 misaligned, context options, the kernel a fused self stage must run on
CASES = [
    ("sf_f32_neusym", [40, 36, 72], "single", R.NEUSYM, UPWIND, False, {}, "k_sf"),              # the BC-on-load march
    ("sf_f64_allneu", [24, 20, 66], "double", R.ALLNEU, UPWIND, False, {}, "k_sf"),
    ("sf_f64_mixed", [21, 19, 34], "double", R.MIXED, UPWIND, False, {}, "k_sf"),
    ("sf_f64_mixed_compat", [21, 19, 34], "double", R.MIXED, COMPAT, False, {}, "k_sf"),
    ("sf_f64_two_row_waves", [80, 6, 32], "double", R.MIXED, UPWIND, False, {}, "k_sf"),
    ("sf_f64_two_row_waves_central", [80, 6, 32], "double", R.ALLDIR, CENTRAL, False, {}, "k_sf"),
    ("sf_f64_one_row_waves", [16, 4, 32], "double", R.MIXED, UPWIND, False, {}, "k_sf"),
    ("sf_f64_one_row_waves_central", [16, 4, 32], "double", R.ALLDIR, CENTRAL, False, {}, "k_sf"),
    ("sf_f64_central_two_ktiles", [12, 20, 136], "double", R.ALLDIR, CENTRAL, False, {}, "k_sf"),   # edge-lane speeds (He)
    ("sf_f32_central_two_ktiles", [9, 40, 264], "single", R.ALLDIR, CENTRAL, False, {}, "k_sf"),
    ("sf_f64_central", [14, 18, 36], "double", R.ALLDIR, CENTRAL, False, {}, "k_sf"),
    ("sf_f64_yperiodic", [16, 20, 40], "double", R.YPER, UPWIND, False, {}, "k_rk_combine"),
    ("sf_f32_central_periodic", [12, 16, 64], "single", R.DIRPER, CENTRAL, False, {}, "k_rk_combine"),
    ("cg3d_f32_odd_rows", [17, 19, 33], "single", R.MIXED, UPWIND, False, {}, "k_cg3d"),
    ("euler_f64_odd_rows_central", [11, 13, 17], "double", R.ALLDIR, CENTRAL, False, {}, "k_euler"),
    ("cg3d_f64_2d", [33, 48], "double", R.MIX2D, UPWIND, False, {}, "k_cg3d"),
    ("euler_f64_2d_central", [33, 48], "double", R.DIR2D, CENTRAL, False, {}, "k_euler"),
    ("euler_f64_1d", [65], "double", R.MIX1D, UPWIND, False, {}, "k_euler"),
    ("cg3d_f32_phi0_misaligned", [40, 36, 72], "single", R.NEUSYM, UPWIND, True, {}, "k_cg3d"),
    ("euler_f64_central_phi0_misaligned", [14, 18, 36], "double", R.ALLDIR, CENTRAL, True, {}, "k_euler"),
    ("cg3d_f32_sf_off", [40, 36, 72], "single", R.NEUSYM, UPWIND, False, {"sf": 0}, "k_cg3d"),
    ("euler_f64_central_sf_off", [14, 18, 36], "double", R.ALLDIR, CENTRAL, False, {"sf": 0}, "k_euler"),
    ("euler_f32_fastpath_off", [40, 36, 72], "single", R.NEUSYM, UPWIND, False, {"fastpath": 0}, "k_euler"),
    ("euler_f64_central_fastpath_off", [12, 20, 136], "double", R.ALLDIR, CENTRAL, False, {"fastpath": 0}, "k_euler"),
]
CASE = {c[0]: c for c in CASES}
# a mesh on which the rule itself selects four rows per wave (sf_rows_per_wave on 256 CUs: 16-row tiles must leave chunks of >= 32
# planes) -- 67 M cells; not the smallest: thin meshes such as [256, 1010, 8] meet the rule with 2 M (tests/test_gpu_chunks.py).
# What runs on it compares a SELF launch with a speed-field launch of the same kernel family, no reference.
RJ4_SHAPE = [256, 512, 512]


def _setup(name, seed=11):
    """test_gpu_rk._setup on this module's cases: mesh, BC config, Div config, (phi_s, phi0) BC-filled, nu, dt"""
    _, n, dtype, bcs, config, misaligned, options, kernel = CASE[name]
    R.CASE["_self_" + name] = ("_self_" + name, n, dtype, bcs, config, 1.0, misaligned, options, kernel)
    try:
        mesh, bc, config, phis, phi0, _, nu, dt = R._setup("_self_" + name, seed)
    finally:
        del R.CASE["_self_" + name]
    return mesh, bc, config, phis, phi0, nu, dt


def _kind(config):
    cfg = config["div"]
    return div_kind(cfg["limiter"], bool(cfg.get("compat", False)))


def _stage(mesh, bc, config, phis, phi0, c0, c1, u, nu, dt):
    """one fused stage (c0 None: the Euler step) with the speed tensor u"""
    ctx = context_for(mesh)
    f = Field("phi", 1, mesh, bc)
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.full_like(phis, float("nan"))
    if c0 is None:
        ctx.euler_step(phis[0], out[0], _kind(config), u, nu, dt)
    else:
        ctx.rk_stage(phis[0], phi0[0], out[0], c0, c1, _kind(config), u, nu, dt)
    return out


def stage_mismatch(mesh, bc, config, phis, phi0, nu, dt):
    """None, or the first (c0, c1) at which the self-advected launch differs from the launch with a clone as the speed"""
    for c0, c1 in [(None, None)] + R.ALL4:
        a = _stage(mesh, bc, config, phis, phi0, c0, c1, phis, nu, dt)            # the same tensor: self-advection
        b = _stage(mesh, bc, config, phis, phi0, c0, c1, phis.clone(), nu, dt)    # a separate speed field with its values
        assert bool(torch.isfinite(b).all())
        if not bit_equal(a, b):
            return (c0, c1, float((a - b).abs().max()), int((a != b).sum()))
    return None


# ---- 1. stage bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_self_stage_is_the_stage_with_a_copy_as_speed_bit_for_bit(name):
    assert stage_mismatch(*_setup(name)) is None


def rj4_case():
    """[256, 512, 512] fp32, random data made on the GPU: upwind with the config-4 BCs, central all-dirichlet"""
    mesh = Mesh(Box[0:1, 0:1, 0:1], None, RJ4_SHAPE, "cuda", "single")
    g = torch.Generator(device="cuda").manual_seed(5)
    dx = min(float(d) for d in mesh.dx_list)
    nu = 1e-3
    dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.3)
    worst = {}
    for bcs, config in ((R.NEUSYM, UPWIND), (R.ALLDIR, CENTRAL)):
        bc = {"domain": mixed_bcs(*bcs), "obstacle": None}
        filled = []
        for _ in range(2):
            f = Field("phi", 1, mesh, bc)
            f.set_var_tensor(torch.rand((1, *RJ4_SHAPE), generator=g, dtype=torch.float32, device="cuda"))
            f.apply_bcs()
            filled.append(f())
        phis, phi0 = filled
        for c0, c1 in ((None, None), (0.75, 0.25)):
            a = _stage(mesh, bc, config, phis, phi0, c0, c1, phis, nu, dt)
            b = _stage(mesh, bc, config, phis, phi0, c0, c1, phis.clone(), nu, dt)
            worst[config["div"]["limiter"], c0] = bool(torch.equal(a, b)) and bool(torch.isfinite(a).all())
            del a, b
    return worst


def test_four_rows_per_wave():
    log = G.child("import torch\nimport test_gpu_self_march as S\n"
                  "w = S.rj4_case(); torch.cuda.synchronize()\n"
                  "assert all(w.values()), w\n")
    lines = [ln for ln in log.splitlines() if "k_sf phase 3" in ln and "(self)" in ln]
    # Euler step and stage, upwind and central: four SELF instantiations, every one at four rows per wave
    assert len(lines) == 4 and all(" RJ 4" in ln for ln in lines), log[-3000:]
    assert sum("kind %d " % div_kind("none", False) in ln for ln in lines) == 2, lines


# ---- 2. paths -------------------------------------------------------------------------------------------------------
def test_paths():
    """the launch log (PYAPES_HIP_DEBUG=1) of one self-advected stage per case and of one march, in ONE child process"""
    code = ("import torch\nimport test_gpu_self_march as S\n"
            "for c in S.CASES:\n"
            "    mesh, bc, config, phis, phi0, nu, dt = S._setup(c[0])\n"
            "    torch.cuda.synchronize(); sys.stderr.write('CASE %s\\n' % c[0]); sys.stderr.flush()\n"
            "    S._stage(mesh, bc, config, phis, phi0, 0.75, 0.25, phis, nu, dt)\n"
            "    torch.cuda.synchronize(); sys.stderr.flush()\n"
            "sys.stderr.write('CASE march\\n'); sys.stderr.flush()\n"
            "S._march('sf_f32_neusym', {}, 3, 2); torch.cuda.synchronize()\n")
    seen = G.case_log(G.child(code), lambda ln: "[pyapes_hip]" in ln)
    for name, *_, kernel in CASES:
        lines = seen[name]
        stage = [ln for ln in lines if "(RK stage" in ln]
        if kernel == "k_sf":
            # (each k_sf case is the first launch of its instantiation, or shares it with at most a few: the log is not exhausted)
            assert len(stage) == 1 and "k_sf phase 3" in stage[0] and "(self)" in stage[0], (name, lines)
            assert not any("k_euler" in ln for ln in lines), (name, lines)
        elif kernel == "k_rk_combine":
            assert len(stage) == 1 and "k_rk_combine" in stage[0], (name, lines)
            step = [ln for ln in lines if "k_sf phase 3" in ln]
            assert len(step) == 1 and "(self)" in step[0] and "(RK stage)" not in step[0], (name, lines)
            assert not any("k_euler" in ln for ln in lines), (name, lines)
        elif stage:   # (a generic / k_cg3d instantiation may have used up its log lines in an earlier case)
            assert len(stage) == 1 and kernel + " " in stage[0] and "(self)" not in stage[0], (name, lines)
    for name in ("cg3d_f32_odd_rows", "euler_f64_odd_rows_central", "cg3d_f64_2d", "euler_f64_1d", "cg3d_f32_phi0_misaligned"):
        assert [ln for ln in seen[name] if "(RK stage" in ln], (name, seen[name])
    # a 2-step order-3 self march on the config-4 BCs: two Euler launches and four fused stages, all BC on load, all SELF
    la = [ln for ln in seen["march"] if "k_sf phase 3" in ln]
    assert len(la) == 6 and all("(BC on load)" in ln and "(self)" in ln for ln in la), seen["march"]
    assert sum("(RK stage)" in ln for ln in la) == 4, seen["march"]
    assert not any("k_euler" in ln for ln in seen["march"]), seen["march"]


# ---- 3. march = pieces that exist without the feature ---------------------------------------------------------------
MARCH_CASES = ["sf_f32_neusym", "sf_f64_mixed", "sf_f64_mixed_compat", "sf_f64_central", "sf_f64_central_two_ktiles",
               "sf_f32_central_two_ktiles", "sf_f64_yperiodic", "sf_f32_central_periodic", "cg3d_f32_odd_rows",
               "euler_f64_odd_rows_central", "cg3d_f64_2d", "euler_f64_1d"]


def _self_march_by_pieces(mesh, bc, config, phi, nu, dt, order, nsteps):
    ctx = context_for(mesh)
    kind = _kind(config)

    def step(phi0):
        return euler_step(G.fresh_field(mesh, bc, phi0), phi0.clone(), nu, dt, config)().clone()

    def stage(cur, phi0, c0, c1):
        f = G.fresh_field(mesh, bc, cur)
        ctx.bind_bcs(f(), f.bcs, 0)
        out = torch.empty_like(cur)
        ctx.rk_stage(cur[0], phi0[0], out[0], c0, c1, kind, cur.clone(), nu, dt)
        return out

    return G.march_by_stages(step, stage, phi, order, nsteps)


@pytest.mark.parametrize("name", MARCH_CASES)
@pytest.mark.parametrize("order", [1, 2, 3])
def test_self_march_is_its_pieces(name, order):
    mesh, bc, config, phis, _, nu, dt = _setup(name)
    for nsteps in (1, 2, 3, 5):
        f = G.fresh_field(mesh, bc, phis, time=True)
        g = rk_march(f, f, nu, dt, nsteps, config, order=order)
        assert g is f
        ref = _self_march_by_pieces(mesh, bc, config, phis, nu, dt, order, nsteps)
        assert bit_equal(f(), ref), (nsteps, float((f() - ref).abs().max()))
        assert f().shape == phis.shape and f().is_contiguous()
        assert abs(float(f.t) - (1.5 + nsteps * dt)) <= 1e-12
        if order == 1:
            e = G.fresh_field(mesh, bc, phis)
            assert euler_march(e, e, nu, dt, nsteps, config) is e and bit_equal(e(), ref)
        h = G.fresh_field(mesh, bc, phis)                     # the field's own tensor as the speed: self-advection as well
        assert bit_equal(rk_march(h, h(), nu, dt, nsteps, config, order=order)(), ref)
    f = G.fresh_field(mesh, bc, phis)
    assert bit_equal(rk_step(f, f, nu, dt, config, order=order)(), _self_march_by_pieces(mesh, bc, config, phis, nu, dt, order, 1))


def test_a_clone_is_a_frozen_speed_as_before():
    mesh, bc, config, phis, _, nu, dt = _setup("sf_f64_mixed")
    u = phis.clone()
    a = rk_march(G.fresh_field(mesh, bc, phis), u, nu, dt, 3, config, order=3)()
    b = R._march_by_stages(mesh, bc, config, phis, u, nu, dt, 3, 3)
    assert bit_equal(a, b) and bit_equal(u, phis)
    f = G.fresh_field(mesh, bc, phis)
    assert not bit_equal(rk_march(f, f, nu, dt, 3, config, order=3)(), a)


# ---- 4. switches ----------------------------------------------------------------------------------------------------
def _march(name, options, order, nsteps):
    mesh, bc, config, phis, _, nu, dt = _setup(name)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    f = G.fresh_field(mesh, bc, phis)
    rk_march(f, f, nu, dt, nsteps, config, order=order)
    return f().clone()


@pytest.mark.parametrize("name", ["sf_f32_neusym", "sf_f64_allneu", "sf_f64_mixed", "sf_f64_two_row_waves", "sf_f64_yperiodic",
                                  "sf_f64_central", "sf_f32_central_two_ktiles", "cg3d_f32_odd_rows"])
@pytest.mark.parametrize("order", [2, 3])
def test_switches_do_not_change_the_bits_of_a_self_march(name, order):
    base = _march(name, {}, order, 4)
    for opt in ({"bcl": 0}, {"sf": 0}, {"fastpath": 0}, {"bcl": 1, "sf": 1, "fastpath": 1}):
        other = _march(name, opt, order, 4)
        assert bit_equal(base, other), (opt, float((base - other).abs().max()))


# ---- 5. order in time -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", [UPWIND, CENTRAL], ids=["upwind", "central"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_order_in_time_of_the_self_march_on_the_gpu(order, config):
    mesh, bc, phi0 = R._pulse_case()
    nu, T = 0.05, 0.02

    def march(n, o):
        f = G.fresh_field(mesh, bc, phi0)
        return rk_march(f, f, nu, T / n, n, config, order=o)().clone()

    ref = march(640, 3)
    err = [float((march(n, order) - ref).abs().max()) for n in (20, 40, 80)]
    ratios = (err[0] / err[1], err[1] / err[2])
    print(f"order {order}: errors {err}, ratios {ratios}")
    lo, hi = H.ORDER_BOUNDS[order]
    for r in ratios:
        assert lo < r < hi, (order, err, ratios)


# ---- 6. Burgers' equation -------------------------------------------------------------------------------------------
def _gpu_burgers(config):
    def march(start, ends, dt, steps):
        n = start.shape[1]
        mesh = Mesh(Box[0:2 * math.pi], None, [n], "cuda", "double")
        bc = {"domain": mixed_bcs(list(ends), ["dirichlet", "dirichlet"]), "obstacle": None}
        f = Field("phi", 1, mesh, bc)
        f.set_var_tensor(start.cuda())
        f.apply_bcs()
        return rk_march(f, f, H.BURGERS_NU, dt, steps, config, order=3)()
    return march


def test_burgers_central_on_the_gpu():
    e1, e2 = (H.burgers_error(n, "none", _gpu_burgers(CENTRAL)) for n in (101, 201))
    print(f"central: {e1:.4e} {e2:.4e} ratio {e1 / e2:.3f}")
    assert e1 <= 2.2e-2 and e1 / e2 >= 3.5, (e1, e2)


def test_burgers_upwind_on_the_gpu():
    e1, e2 = (H.burgers_error(n, "upwind", _gpu_burgers(UPWIND)) for n in (101, 201))
    print(f"upwind: {e1:.4e} {e2:.4e} ratio {e1 / e2:.3f}")
    assert 1.6 < e1 / e2 < 2.2, (e1, e2)


# ---- 7. errors ------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    mesh, bc, config, phis, phi0, nu, dt = _setup("sf_f64_mixed")
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, phis)
    ctx.bind_bcs(f(), f.bcs, 0)
    kind = div_kind("upwind", False)
    w1, w2 = torch.empty_like(phis), torch.empty_like(phis)
    with pytest.raises(PaError):
        ctx.rk_march_self(phis[0], w1[0], w1[0], 3, kind, nu, dt, 2)             # w1 is w2
    with pytest.raises(PaError):
        ctx.rk_march_self(phis[0], phis[0], w2[0], 3, kind, nu, dt, 2)           # w1 is phi
    with pytest.raises(PaError):
        ctx.rk_march_self(phis[0], w1[0], phis[0], 2, kind, nu, dt, 2)           # w2 is phi
    with pytest.raises(PaError):
        ctx.rk_march_self(phis[0], w1[0], None, 2, kind, nu, dt, 2)              # no w2 above order 1
    with pytest.raises(PaError):
        ctx.rk_march_self(phis[0], phis[0], None, 1, kind, nu, dt, 2)            # order 1: w1 is phi
    with pytest.raises(PaError):
        ctx.rk_march_self(phis[0], w1[0], w2[0], 0, kind, nu, dt, 2)             # order 0 at the C ABI
    with pytest.raises(PaError):
        ctx.rk_march_self(phis[0], w1[0], w2[0], 3, 99, nu, dt, 2)               # bad Div kind
    with pytest.raises(PaError):
        ctx.rk_march_self(phis[0], w1[0], w2[0], 3, kind, nu, dt, -1)
    assert bit_equal(ctx.rk_march_self(phis[0], w1[0], None, 1, kind, nu, dt, 0), phis[0])   # order 1 needs no w2
    # slab mode at the C ABI: PA_E_STATE with a message
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    sctx = context_for(slab)
    sphi = torch.zeros(tuple(slab.nx), dtype=torch.float64, device="cuda")
    sf = Field("phi", 1, slab, {"domain": mixed_bcs(*R.MIXED), "obstacle": None})
    with pytest.raises(PaError, match="single GPU"):
        sctx.rk_march_self(sphi, torch.empty_like(sphi), torch.empty_like(sphi), 3, kind, nu, dt, 2)
    # in Python: a slab mesh or a vector field
    with pytest.raises(NotImplementedError):
        rk_march(sf, sf, nu, dt, 2, config)
    with pytest.raises(NotImplementedError):
        euler_march(sf, sf, nu, dt, 2, config)
    vec = Field("v", 3, mesh, {"domain": mixed_bcs(*R.MIXED), "obstacle": None})
    with pytest.raises(NotImplementedError):
        rk_march(vec, vec, nu, dt, 2, config)
    with pytest.raises(NotImplementedError):
        euler_march(vec, vec, nu, dt, 2, config)
    # the context that saw the errors still steps, and gives what a fresh one gives
    g = G.fresh_field(mesh, bc, phis)
    a = rk_march(g, g, nu, dt, 2, config)().clone()
    mesh_b, bc_b, _, phis_b, _, _, _ = _setup("sf_f64_mixed")
    h = G.fresh_field(mesh_b, bc_b, phis_b)
    b = rk_march(h, h, nu, dt, 2, config)()
    assert bit_equal(phis, phis_b) and bit_equal(a, b)
