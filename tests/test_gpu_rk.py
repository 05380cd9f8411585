"""-m gpu: SSP Runge-Kutta stages fused into the Euler step kernels (pa_rk_stage / pa_rk_march; csrc STG variants of k_sf,
k_cg3d phase 3 and k_euler).

The yardstick is the composition of public pieces that exist without the feature:
    E = euler_step(copy of phi_s);  C = (c0 * phi0) + (c1 * E)  as three torch ops in the mesh dtype;  apply_bcs(C)
and a fused stage must give those BITS -- on every kernel path, for every Div scheme, for both signs of a scalar speed, a
speed tensor, the BC mixes of test_gpu_bcl.py and a periodic axis, the (c0, c1) of every fused stage, and a phi0 that is
not 16-byte aligned (which must fall to the next path).  (With a periodic face the stage cannot be ONE kernel -- the
periodic fill reads a face value before it rewrites it, csrc/pa_march.hip step_t -- and runs as step + combine kernel.)  The march must be its stages, the kernel switches must not change
bits, and the facts tests/test_rk_host.py establishes on the CPU (order in time, stability of central advection) must hold
through rk_march on the GPU with the same bounds.
"""
import pytest
import torch

import march_gpu as G
from helpers import bit_equal, offset_view
from march_gpu import ALLDIR, MIXED
from pyapes_amd.geometry import Box
from pyapes_amd.hip.context import context_for
from pyapes_amd.hip.lib import PaError
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.march import SSP_STAGES, euler_march, euler_step, rk_march, rk_step
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

NEUSYM = ([0.0, 0.0, None, None, None, None], ["neumann", "neumann", "symmetry", "symmetry", "symmetry", "symmetry"])
ALLNEU = ([0.3, -0.2, 0.1, 0.0, -0.4, 0.25], ["neumann"] * 6)
YPER = ([0.5, 0.1, None, None, -0.3, None], ["dirichlet", "neumann", "periodic", "periodic", "neumann", "symmetry"])
DIRPER = ([0.0, 1.0, None, None, None, None], ["dirichlet", "dirichlet", "periodic", "periodic", "periodic", "periodic"])
DIR2D = ([0.0, 1.0, 0.25, -0.5], ["dirichlet"] * 4)
MIX2D = ([0.5, 0.1, None, 1.0], ["dirichlet", "neumann", "symmetry", "dirichlet"])
MIX1D = ([0.5, 0.1], ["dirichlet", "neumann"])
PER1D = ([None, None], ["periodic", "periodic"])

UPWIND = {"div": {"limiter": "upwind"}}
COMPAT = {"div": {"limiter": "upwind", "compat": True}}
CENTRAL = {"div": {"limiter": "none"}}
# (c0, c1) of the fused stages: the three of the stage table (order 3: (3/4, 1/4), (1/3, 2/3); order 2: (1/2, 1/2)) and one
# more pair with the small weight on phi0
ALL4 = [(0.75, 0.25), (1.0 / 3.0, 2.0 / 3.0), (0.5, 0.5), (0.25, 0.75)]

# name, n, dtype, bcs, config, u, phi0 misaligned, context options, the kernel a fused stage must run on
CASES = [
    ("sf_f32_config4", [40, 36, 72], "single", NEUSYM, UPWIND, 1.0, False, {}, "k_sf"),
    ("sf_f64_allneu_uneg", [24, 20, 66], "double", ALLNEU, UPWIND, -0.8, False, {}, "k_sf"),
    ("sf_f64_mixed", [21, 19, 34], "double", MIXED, UPWIND, 0.6, False, {}, "k_sf"),
    ("sf_f32_alldir", [18, 22, 132], "single", ALLDIR, UPWIND, 1.3, False, {}, "k_sf"),
    ("sf_f32_speed_field", [20, 24, 64], "single", NEUSYM, UPWIND, "field", False, {}, "k_sf"),
    ("sf_f64_two_row_waves", [80, 6, 32], "double", MIXED, UPWIND, 1.0, False, {}, "k_sf"),
    ("sf_f64_yperiodic", [16, 20, 40], "double", YPER, UPWIND, -1.1, False, {}, "k_rk_combine"),
    ("sf_f32_compat", [18, 20, 64], "single", MIXED, COMPAT, 0.7, False, {}, "k_sf"),
    ("sf_f32_compat_field", [18, 20, 64], "single", MIXED, COMPAT, "field", False, {}, "k_sf"),
    ("sf_f64_central", [14, 18, 36], "double", ALLDIR, CENTRAL, -0.9, False, {}, "k_sf"),
    ("sf_f32_central_periodic", [12, 16, 64], "single", DIRPER, CENTRAL, 1.2, False, {}, "k_rk_combine"),
    ("cg3d_f32_odd_rows", [17, 19, 33], "single", MIXED, UPWIND, 0.9, False, {}, "k_cg3d"),
    ("cg3d_f64_odd_rows_field", [13, 17, 35], "double", ALLNEU, UPWIND, "field", False, {}, "k_cg3d"),
    ("cg3d_f64_odd_rows_central", [11, 13, 17], "double", ALLDIR, CENTRAL, 0.8, False, {}, "k_cg3d"),
    ("cg3d_f64_2d", [33, 48], "double", MIX2D, UPWIND, -0.7, False, {}, "k_cg3d"),
    ("cg3d_f32_2d_compat", [40, 64], "single", DIR2D, COMPAT, 1.0, False, {}, "k_cg3d"),
    ("cg3d_f32_phi0_misaligned", [40, 36, 72], "single", NEUSYM, UPWIND, 1.0, True, {}, "k_cg3d"),
    ("cg3d_f64_phi0_misaligned", [21, 19, 34], "double", MIXED, UPWIND, -0.6, True, {}, "k_cg3d"),
    ("cg3d_f32_sf_off", [18, 22, 132], "single", ALLDIR, UPWIND, 1.3, False, {"sf": 0}, "k_cg3d"),
    ("euler_f64_1d", [65], "double", MIX1D, UPWIND, 0.8, False, {}, "k_euler"),
    ("euler_f32_1d_periodic_central", [64], "single", PER1D, CENTRAL, -1.0, False, {}, "k_rk_combine"),
    ("euler_f64_central_field", [12, 14, 16], "double", ALLDIR, CENTRAL, "field", False, {}, "k_euler"),
    ("euler_f32_fastpath_off", [18, 22, 132], "single", MIXED, UPWIND, 1.3, False, {"fastpath": 0}, "k_euler"),
]
CASE = {c[0]: c for c in CASES}


def _setup(name, seed=9):
    """mesh, BC config, (phi_s, phi0) BC-filled fields' tensors, the speed, nu, dt"""
    _, n, dtype, bcs, config, u, misaligned, options, _ = CASE[name]
    mesh = Mesh(G.box(len(n)), None, n, "cuda", dtype)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    g = torch.Generator().manual_seed(seed)
    raw = [torch.rand((1, *n), generator=g, dtype=torch.float64) for _ in range(2)]
    ufield = torch.randn((1, *n), generator=g, dtype=torch.float64).to(mesh.dtype.float).cuda()
    bc = {"domain": mixed_bcs(*bcs), "obstacle": None}
    filled = []
    for r in raw:
        f = Field("phi", 1, mesh, bc)
        f.set_var_tensor(r.to(mesh.dtype.float).cuda())
        f.apply_bcs()
        filled.append(f().clone())
    phis, phi0 = filled
    if misaligned:   # a contiguous view one element into a larger allocation: not 16-byte aligned
        shape, values = phi0.shape, phi0.clone()
        phi0, _ = offset_view(phi0, 1)
        assert phi0.is_contiguous() and phi0.data_ptr() % 16 != 0
        assert phi0.shape == shape and phi0.is_cuda and torch.equal(phi0, values)
    dx = min(float(d) for d in mesh.dx_list)
    nu = 1e-3
    dt = 0.2 * min(dx * dx / (2 * len(n) * nu), dx / 1.3)
    return mesh, bc, config, phis, phi0, (ufield if u == "field" else u), nu, dt


def _composition(mesh, bc, config, phis, phi0, c0, c1, u, nu, dt):
    f = Field("phi", 1, mesh, bc)
    f.set_var_tensor(phis.clone())
    e = euler_step(f, u, nu, dt, config)()
    t0 = c0 * phi0
    t1 = c1 * e
    c = t0 + t1
    assert c.dtype == mesh.dtype.float
    f.set_var_tensor(c)
    f.apply_bcs()
    return f()


def _fused(mesh, bc, config, phis, phi0, c0, c1, u, nu, dt):
    from pyapes_amd.solver.fdc import div_kind
    cfg = config["div"]
    ctx = context_for(mesh)
    f = Field("phi", 1, mesh, bc)
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.full_like(phis, float("nan"))
    ctx.rk_stage(phis[0], phi0[0], out[0], c0, c1, div_kind(cfg["limiter"], bool(cfg.get("compat", False))), u, nu, dt)
    return out


def run_stage_case(name):
    mesh, bc, config, phis, phi0, u, nu, dt = _setup(name)
    worst = None
    for c0, c1 in ALL4:
        a = _fused(mesh, bc, config, phis, phi0, c0, c1, u, nu, dt)
        b = _composition(mesh, bc, config, phis, phi0, c0, c1, u, nu, dt)
        if not bit_equal(a, b):
            worst = (c0, c1, float((a - b).abs().max()), int((a != b).sum()))
            break
    return worst


def test_the_case_constants_are_the_stage_table():
    table = [s for o in (2, 3) for s in SSP_STAGES[o]]
    for s in table:
        assert s in ALL4
    assert len(ALL4) == 4 and all(abs(a + b - 1) < 1e-15 for a, b in ALL4)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_stage_is_the_composition_bit_for_bit(name):
    assert run_stage_case(name) is None


def test_every_case_runs_on_the_kernel_it_is_meant_for():
    """the launch log (PYAPES_HIP_DEBUG=1) of one fused stage per case, in ONE child process (the log is limited per kernel
    instantiation, so every case prints a marker line first and only the lines behind it are read)"""
    code = ("import torch\nimport test_gpu_rk as R\n"
            "for c in R.CASES:\n"
            "    mesh, bc, config, phis, phi0, u, nu, dt = R._setup(c[0])\n"
            "    torch.cuda.synchronize(); sys.stderr.write('CASE %s\\n' % c[0]); sys.stderr.flush()\n"
            "    R._fused(mesh, bc, config, phis, phi0, 0.75, 0.25, u, nu, dt)\n"
            "    torch.cuda.synchronize(); sys.stderr.flush()\n")
    seen = G.case_log(G.child(code), lambda ln: "(RK stage" in ln)
    kernels_hit = set()
    for name, *_, kernel in CASES:
        lines = seen.get(name, [])
        if not lines:
            # the log of an instantiation is limited to its first launches: a case may share one with an earlier case
            continue
        assert len(lines) == 1 and kernel + " " in lines[0], (name, kernel, lines)
        kernels_hit.add(kernel)
    assert kernels_hit == {"k_sf", "k_cg3d", "k_euler", "k_rk_combine"}, seen
    # the cases that exist to show a fall-back must have been seen themselves
    for name in ("cg3d_f32_phi0_misaligned", "cg3d_f64_phi0_misaligned", "cg3d_f32_odd_rows", "cg3d_f64_2d", "euler_f64_1d",
                 "euler_f64_central_field", "sf_f32_config4", "sf_f64_allneu_uneg"):
        assert seen.get(name), (name, seen)


# ---- march = stages -------------------------------------------------------------------------------------------------
MARCH_CASES = ["sf_f32_config4", "sf_f64_mixed", "sf_f64_yperiodic", "cg3d_f32_odd_rows", "cg3d_f64_2d", "euler_f64_1d",
               "sf_f32_speed_field", "sf_f64_central"]


def _march_by_stages(mesh, bc, config, phi, u, nu, dt, order, nsteps):
    from pyapes_amd.solver.fdc import div_kind
    cfg = config["div"]
    kind = div_kind(cfg["limiter"], bool(cfg.get("compat", False)))
    ctx = context_for(mesh)

    def step(phi0):
        return euler_step(G.fresh_field(mesh, bc, phi0), u, nu, dt, config)().clone()

    def stage(cur, phi0, c0, c1):
        f = G.fresh_field(mesh, bc, cur)
        ctx.bind_bcs(f(), f.bcs, 0)
        out = torch.empty_like(cur)
        ctx.rk_stage(cur[0], phi0[0], out[0], c0, c1, kind, u, nu, dt)
        return out

    return G.march_by_stages(step, stage, phi, order, nsteps)


@pytest.mark.parametrize("name", MARCH_CASES)
@pytest.mark.parametrize("order", [1, 2, 3])
def test_march_is_its_stages(name, order):
    mesh, bc, config, phis, _, u, nu, dt = _setup(name)
    for nsteps in (1, 2, 3, 5):
        f = G.fresh_field(mesh, bc, phis, time=True)
        g = rk_march(f, u, nu, dt, nsteps, config, order=order)
        assert g is f                                    # the field handed in holds the result ...
        ref = _march_by_stages(mesh, bc, config, phis, u, nu, dt, order, nsteps)
        assert bit_equal(f(), ref), (nsteps, float((f() - ref).abs().max()))   # ... i.e. the right one of the three buffers
        assert f().shape == phis.shape and f().is_contiguous()
        if order == 1:
            e = euler_march(G.fresh_field(mesh, bc, phis), u, nu, dt, nsteps, config)
            assert bit_equal(f(), e())
        assert abs(float(f.t) - (1.5 + nsteps * dt)) <= 1e-12
        g = rk_march(G.fresh_field(mesh, bc, phis), u, nu, dt, nsteps, config, order=order)   # no time set: nothing to advance
        assert bit_equal(g(), ref)
    # one step through rk_step
    f = rk_step(G.fresh_field(mesh, bc, phis), u, nu, dt, config, order=order)
    assert bit_equal(f(), _march_by_stages(mesh, bc, config, phis, u, nu, dt, order, 1))


# ---- switches -------------------------------------------------------------------------------------------------------
def _march_with(name, options, order, nsteps):
    mesh, bc, config, phis, _, u, nu, dt = _setup(name)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    f = G.fresh_field(mesh, bc, phis)
    rk_march(f, u, nu, dt, nsteps, config, order=order)
    return f().clone()


@pytest.mark.parametrize("name", ["sf_f32_config4", "sf_f64_allneu_uneg", "sf_f64_mixed", "sf_f32_speed_field",
                                  "sf_f64_two_row_waves", "sf_f64_yperiodic", "sf_f64_central", "cg3d_f32_odd_rows"])
@pytest.mark.parametrize("order", [2, 3])
def test_switches_do_not_change_bits(name, order):
    base = _march_with(name, {}, order, 4)
    for opt in ({"bcl": 0}, {"sf": 0}, {"fastpath": 0}, {"bcl": 1, "sf": 1, "fastpath": 1}):
        other = _march_with(name, opt, order, 4)
        assert bit_equal(base, other), (opt, float((base - other).abs().max()))


def test_bc_on_load_is_taken_for_all_stages_and_declined_with_a_periodic_face():
    code = ("import torch\nimport test_gpu_rk as R\n"
            "sys.stderr.write('CASE a\\n'); sys.stderr.flush()\n"
            "R._march_with('sf_f32_config4', {}, 3, 2); torch.cuda.synchronize()\n"
            "sys.stderr.write('CASE b\\n'); sys.stderr.flush()\n"
            "R._march_with('sf_f64_yperiodic', {}, 3, 2); torch.cuda.synchronize()\n")
    seen = G.case_log(G.child(code), lambda ln: "k_sf phase 3" in ln or "k_rk_combine (RK stage" in ln)
    la = [ln for ln in seen["a"] if "k_sf phase 3" in ln]
    lb = [ln for ln in seen["b"] if "k_sf phase 3" in ln]
    # two steps of three launches: two Euler launches and four fused stages, every one in the BC-on-load form
    assert len(la) == 6 and all("(BC on load)" in ln for ln in la), la
    assert sum("(RK stage)" in ln for ln in la) == 4, la
    # a periodic face: no BC on load, and every stage is the step kernel + the combine kernel
    assert len(lb) == 6 and not any("(BC on load)" in ln or "(RK stage)" in ln for ln in lb), lb
    assert sum("k_rk_combine (RK stage" in ln for ln in seen["b"]) == 4, seen["b"]


# ---- the CPU facts of tests/test_rk_host.py, through rk_march -------------------------------------------------------
ORDER_BOUNDS = {1: (1.7, 2.4), 2: (3.4, 4.8), 3: (6.8, 9.6)}


def _pulse_case():
    mesh = Mesh(Box[0:1, 0:1], None, [33, 33], "cuda", "double")
    bc = {"domain": mixed_bcs([0.0] * 4, ["dirichlet"] * 4), "obstacle": None}
    x, y = mesh.grid
    f = Field("phi", 1, mesh, bc)
    f.set_var_tensor(torch.exp(-((x - 0.4) ** 2 + (y - 0.5) ** 2) / 0.01).unsqueeze(0).to(mesh.dtype.float))
    f.apply_bcs()
    return mesh, bc, f().clone()


@pytest.mark.parametrize("config", [UPWIND, CENTRAL], ids=["upwind", "central"])
@pytest.mark.parametrize("order", [2, 3])
def test_order_in_time_on_the_gpu(order, config):
    mesh, bc, phi0 = _pulse_case()
    u, nu, T = 1.0, 0.05, 0.02
    ref = rk_march(G.fresh_field(mesh, bc, phi0), u, nu, T / 640, 640, config, order=3)().clone()
    err = [float((rk_march(G.fresh_field(mesh, bc, phi0), u, nu, T / n, n, config, order=order)() - ref).abs().max())
           for n in (20, 40, 80)]
    ratios = (err[0] / err[1], err[1] / err[2])
    print(f"order {order}: errors {err}, ratios {ratios}")
    lo, hi = ORDER_BOUNDS[order]
    for r in ratios:
        assert lo < r < hi, (order, err, ratios)


def test_central_advection_without_diffusion_on_the_gpu():
    mesh, bc, phi0 = _pulse_case()
    top = float(phi0.abs().max())
    dx = float(mesh.dx_list[0])
    ends = {}
    for cfl, steps in ((1.0, 8), (1.5, 5)):
        for order in (1, 2, 3):
            ends[cfl, order] = float(rk_march(G.fresh_field(mesh, bc, phi0), 1.0, 0.0, cfl * dx, steps, CENTRAL, order=order)().abs().max())
    print("max|phi| at the end:", ends)
    assert ends[1.0, 3] <= top and ends[1.5, 3] <= top, ends
    assert ends[1.0, 1] >= 2 * top, ends


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    from pyapes_amd.solver.fdc import div_kind
    mesh, bc, config, phis, phi0, u, nu, dt = _setup("sf_f64_mixed")
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, phis)
    ctx.bind_bcs(f(), f.bcs, 0)
    kind = div_kind("upwind", False)
    out = torch.empty_like(phis)
    with pytest.raises(PaError):
        ctx.rk_stage(phis[0], phi0[0], phis[0], 0.5, 0.5, kind, u, nu, dt)       # out is phi
    with pytest.raises(PaError):
        ctx.rk_stage(phis[0], phi0[0], phi0[0], 0.5, 0.5, kind, u, nu, dt)       # out is phi0
    with pytest.raises(PaError):
        ctx.rk_march(phis[0], out[0], out[0], 3, kind, u, nu, dt, 2)             # w1 is w2
    with pytest.raises(PaError):
        ctx.rk_march(phis[0], phis[0], out[0], 3, kind, u, nu, dt, 2)            # w1 is phi
    with pytest.raises(PaError):
        ctx.rk_march(phis[0], out[0], torch.empty_like(out)[0], 0, kind, u, nu, dt, 2)   # order 0 at the C ABI
    with pytest.raises(PaError):
        ctx.rk_march(phis[0], out[0], torch.empty_like(out)[0], 3, 99, u, nu, dt, 2)     # bad Div kind
    with pytest.raises(ValueError):
        rk_march(G.fresh_field(mesh, bc, phis), u, nu, dt, 2, config, order=0)
    with pytest.raises(ValueError):
        rk_step(G.fresh_field(mesh, bc, phis), u, nu, dt, config, order=4)
    vec = Field("v", 3, mesh, {"domain": mixed_bcs(*MIXED), "obstacle": None})
    with pytest.raises(NotImplementedError):
        rk_march(vec, u, nu, dt, 2, config)
    mesh2 = Mesh(Box[0:1, 0:1], None, [16, 16], "cuda", "double")
    vec2 = Field("v", 2, mesh2, {"domain": mixed_bcs(*DIR2D), "obstacle": None})
    assert vec2.dim == 2
    with pytest.raises(NotImplementedError):
        rk_march(vec2, 1.0, nu, dt, 2, UPWIND)
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    sf = Field("phi", 1, slab, {"domain": mixed_bcs(*MIXED), "obstacle": None})
    with pytest.raises(NotImplementedError):
        rk_march(sf, u, nu, dt, 2, config)
    with pytest.raises(NotImplementedError):
        rk_step(sf, u, nu, dt, config)
    # the context that saw the errors still steps, and gives what a fresh one gives
    a = euler_step(G.fresh_field(mesh, bc, phis), u, nu, dt, config)().clone()
    mesh_b, bc_b, _, phis_b, _, _, _, _ = _setup("sf_f64_mixed")
    b = euler_step(G.fresh_field(mesh_b, bc_b, phis_b), u, nu, dt, config)()
    assert bit_equal(phis, phis_b) and bit_equal(a, b)
