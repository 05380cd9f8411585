"""-m gpu: the marches in a velocity field -- one advection speed per mesh axis: a tuple / (dim, *n) tensor / vector Field as
``u`` of euler_step / euler_march / rk_step / rk_march, pa_*_vel at the C ABI, the VEL instantiations of k_sf (upwind, three
scalar speeds or three speed fields) and of the generic k_euler (everything else).

The yardstick is tests/march_ref.py, the step in a velocity restated on the CPU operation for operation, and the device must give its
BITS: on both kernels, for the three Div limiters, scalar and field velocities of mixed signs with three DISTINCT components (a
swapped axis cannot pass), Dirichlet and mixed faces, no source / a source field / a scalar source, the Euler step and both
fused stages of order 3.  Meshes as tests/test_gpu_source.py: whole 16-byte rows and two k tiles (132 fp64 / 260 fp32 nodes per
row), n1 = 13 / 14, n0 = 7 / 9 with the chunk cap at 1, 2, 3; the generic kernel's odd rows in 3-D, 2-D, 1-D; a periodic axis
0.  (The row-count, row-length and periodic-axis edges of the two-row VEL kernels -- n1 = 5 .. 36 with 8 / 9 / 16 / 17 among them,
rows of 2 * VEC to 264 nodes, a periodic axis 1 or 2, all-Neumann faces, long chunks -- are swept in
tests/test_gpu_chunks_terms.py.)  The exact shift needs no reference at all: with dx = dt = 1 and u = +-e_a one upwind step moves small integers by one node.
"""
import ctypes as C

import pytest
import torch

import march_gpu as G
import march_ref as R
from helpers import bit_equal
from march_gpu import GENERIC, LIMITER_BCS, VECTOR, VECTOR_OPTIONS
from pyapes_amd.geometry import Box, Cylinder
from pyapes_amd.hip import lib as L
from pyapes_amd.hip.context import context_for
from pyapes_amd.hip.lib import PaError
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import div_kind
from pyapes_amd.solver.march import SSP_STAGES, euler_march, euler_step, rk_march, rk_step
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

STAGES3 = SSP_STAGES[3]
SCALARS = (0.9, -0.8, 0.4)                        # mixed signs, three distinct speeds
SCALAR_SOURCE = 1.75

_ids = G.mesh_id


def _setup(n, dtype, bcname):
    """march_gpu.setup with a velocity (nd, *n) of distinct random components in place of the one speed field"""
    return G.setup(n, dtype, bcname, len(n))


def _vels(which, vel_c):
    """(the reference's velocity, the device's): per-axis numbers, or per-axis tensors"""
    nd = vel_c.shape[0]
    if which == "scalar":
        return list(SCALARS[:nd]), list(SCALARS[:nd])
    vd = vel_c.cuda()
    return [vel_c[a] for a in range(nd)], [vd[a] for a in range(nd)]


def _gpu_launch(mesh, bc, phi_d, phi0_d, stage, kind, vel_d, nu, dt, source):
    """one Euler step (stage None) or fused stage through the Context, the BCs bound; returns the (1, *n) result"""
    ctx = context_for(mesh)
    f = Field("phi", 1, mesh, bc)
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.full_like(phi_d, float("nan"))
    if stage is None:
        ctx.euler_step_vel(phi_d[0], out[0], kind, vel_d, nu, dt, source=source)
    else:
        ctx.rk_stage_vel(phi_d[0], phi0_d[0], out[0], stage[0], stage[1], kind, vel_d, nu, dt, source=source)
    return out


def run_case(n, dtype, limiter, option_sets, bcnames=None):
    kind = div_kind(limiter, False)
    bad = []
    for bcname in bcnames or LIMITER_BCS[limiter]:
        mesh, bc, om, obcs, phi_c, phi0_c, vel_c, src_c, nu, dt = _setup(n, dtype, bcname)
        ctx = context_for(mesh)
        phi_d, phi0_d, src_d = phi_c.cuda(), phi0_c.cuda(), src_c.cuda()
        for which in ("scalar", "field"):
            v_ref, v_dev = _vels(which, vel_c)
            for stage in (None, *STAGES3):
                for sname, s_ref, s_dev in ((None, None, None), ("field", src_c, src_d[0]), ("scalar", SCALAR_SOURCE, SCALAR_SOURCE)):
                    if stage is None:
                        want = R.euler_step(phi_c, v_ref, nu, dt, om, obcs, limiter, s_ref)
                    else:
                        want = R.rk_stage(phi_c, phi0_c, stage[0], stage[1], v_ref, nu, dt, om, obcs, limiter, s_ref)
                    for opts in option_sets:
                        for k, v in opts.items():
                            ctx.set_option(k, v)
                        got = _gpu_launch(mesh, bc, phi_d, phi0_d, stage, kind, v_dev, nu, dt, s_dev)
                        if not bit_equal(got, want):
                            bad.append((bcname, which, stage, sname, opts, float((got.cpu() - want).abs().max())))
        ctx.set_option("sf", 1)
        ctx.set_option("chunks", 0)
    return bad


@pytest.mark.parametrize("n,dtype", VECTOR, ids=_ids)
def test_upwind_step_and_stage_on_the_vector_kernel(n, dtype):
    assert run_case(n, dtype, "upwind", VECTOR_OPTIONS) == []


@pytest.mark.parametrize("limiter", ["upwind", "quick", "none", "minmod", "mc"])
@pytest.mark.parametrize("n,dtype", GENERIC, ids=_ids)
def test_step_and_stage_on_the_generic_kernel(n, dtype, limiter):
    assert run_case(n, dtype, limiter, [{}]) == []


@pytest.mark.parametrize("limiter", ["upwind", "quick", "none", "minmod", "mc"])
def test_step_and_stage_with_a_periodic_axis_0(limiter):
    """the stage is the step, then k_rk_combine, then the fill; the velocity takes the generic kernel"""
    assert run_case([9, 14, 132], "double", limiter, [{}], bcnames=("xper",)) == []


@pytest.mark.parametrize("limiter", ["quick", "none"])
@pytest.mark.parametrize("n,dtype", VECTOR, ids=_ids)
def test_quick_and_central_on_the_vector_meshes(n, dtype, limiter):
    """no VEL instantiation of k_sfq or of central k_sf: the generic kernel"""
    assert run_case(n, dtype, limiter, [{}]) == []


# ---- equal components are today's call ------------------------------------------------------------------------------
@pytest.mark.parametrize("limiter", ["upwind", "quick", "none"])
@pytest.mark.parametrize("n,dtype", [([9, 14, 260], "single"), ([6, 7, 9], "double")], ids=["vector", "generic"])
def test_equal_components_are_todays_call(n, dtype, limiter):
    bcname = LIMITER_BCS[limiter][-1]
    mesh, bc, _, _, phi_c, _, vel_c, _, nu, dt = _setup(n, dtype, bcname)
    cfg = G.config(limiter)
    U = vel_c.cuda()[0:1].contiguous()
    for c in (0.9, -0.8):
        assert bit_equal(euler_step(G.fresh_field(mesh, bc, phi_c), (c, c, c), nu, dt, cfg)(), euler_step(G.fresh_field(mesh, bc, phi_c), c, nu, dt, cfg)())
        assert bit_equal(rk_march(G.fresh_field(mesh, bc, phi_c), (c, c, c), nu, dt, 3, cfg, order=3)(),
                         rk_march(G.fresh_field(mesh, bc, phi_c), c, nu, dt, 3, cfg, order=3)())
    assert bit_equal(euler_step(G.fresh_field(mesh, bc, phi_c), (U[0], U[0], U[0]), nu, dt, cfg)(), euler_step(G.fresh_field(mesh, bc, phi_c), U, nu, dt, cfg)())
    assert bit_equal(rk_march(G.fresh_field(mesh, bc, phi_c), (U[0], U[0], U[0]), nu, dt, 3, cfg, order=3)(),
                     rk_march(G.fresh_field(mesh, bc, phi_c), U, nu, dt, 3, cfg, order=3)())


# ---- exact shift ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["single", "double"])
@pytest.mark.parametrize("fastpath", [1, 0], ids=["k_sf", "fastpath0"])
def test_exact_shift(fastpath, dtype):
    """dx = 1 on every axis, small integers, nu = 0, dt = 1, dirichlet faces: u = +e_a shifts the field by one node along a on
    the interior set, exactly; -e_a the other way.  No oracle involved."""
    n = [9, 14, 132]
    mesh = Mesh(Box[0:8, 0:13, 0:131], None, n, "cuda", dtype)
    assert all(abs(float(d) - 1.0) < 1e-15 for d in mesh.dx_list)
    context_for(mesh).set_option("fastpath", fastpath)
    bc = {"domain": mixed_bcs([2.0] * 6, ["dirichlet"] * 6), "obstacle": None}
    g = torch.Generator().manual_seed(7)
    phi = torch.randint(-8, 9, (1, *n), generator=g).to(mesh.dtype.float).cuda()
    inner = (slice(1, -1),) * 3
    for axis in range(3):
        for sign in (1.0, -1.0):
            u = [0.0, 0.0, 0.0]
            u[axis] = sign
            want = torch.roll(phi[0], 1 if sign > 0 else -1, axis)
            for vel in (tuple(u), tuple(torch.full_like(phi[0], v) for v in u)):
                f = Field("phi", 1, mesh, bc)
                f.set_var_tensor(phi.clone())
                got = euler_step(f, vel, 0.0, 1.0, G.config("upwind"))()
                assert torch.equal(got[0][inner], want[inner]), (axis, sign)


# ---- routing --------------------------------------------------------------------------------------------------------
# name, mesh, dtype, BCs, limiter, velocity, source, options -> the kernel a step and a stage must run on.  The launch log is
# limited per kernel instantiation: the k_sf routes use distinct instantiations (dtype x VEL x source)
ROUTES = [
    ("sf_scalar_f64", [9, 14, 132], "double", "mix", "upwind", "scalar", None, {"sf": 2}, "k_sf"),
    ("sf_field_f64", [7, 13, 132], "double", "dir", "upwind", "field", None, {"sf": 4}, "k_sf"),
    ("sf_scalar_src_f64", [9, 14, 132], "double", "dir", "upwind", "scalar", "field", {}, "k_sf"),
    ("sf_field_src_f64", [9, 14, 132], "double", "mix", "upwind", "field", "scalar", {"chunks": 2}, "k_sf"),
    ("sf_scalar_f32", [7, 13, 260], "single", "mix", "upwind", "scalar", None, {"sf": 4}, "k_sf"),
    ("sf_field_f32", [9, 14, 260], "single", "mix", "upwind", "field", None, {"sf": 2}, "k_sf"),
    ("sf_scalar_src_f32", [9, 14, 260], "single", "mix", "upwind", "scalar", "scalar", {}, "k_sf"),
    ("sf_field_src_f32", [9, 14, 260], "single", "dir", "upwind", "field", "field", {}, "k_sf"),
    ("gen_central_f64", [9, 14, 132], "double", "dir", "none", "field", None, {}, "k_euler"),
    ("gen_quick_f32", [9, 14, 260], "single", "mix", "quick", "scalar", None, {}, "k_euler"),
    ("gen_quick_field_f64", [7, 13, 132], "double", "mix", "quick", "field", "field", {}, "k_euler"),
    ("gen_odd_rows_f64", [6, 7, 9], "double", "mix", "upwind", "field", None, {}, "k_euler"),
    ("gen_2d_f64", [17, 12], "double", "mix", "upwind", "scalar", "field", {}, "k_euler"),
    ("gen_1d_f32", [33], "single", "mix", "upwind", "field", None, {}, "k_euler"),
    ("gen_sf_off_f64", [9, 14, 132], "double", "mix", "upwind", "scalar", None, {"sf": 0}, "k_euler"),
    ("gen_fastpath_off_f32", [9, 14, 260], "single", "mix", "upwind", "field", None, {"fastpath": 0}, "k_euler"),
    ("gen_xper_f64", [9, 14, 132], "double", "xper", "upwind", "scalar", None, {}, "k_euler"),
]


def route_case(name, stage):
    """one launch of the named route (a fresh mesh, so that its options are its own)"""
    _, n, dtype, bcname, limiter, which, source, options, _ = next(r for r in ROUTES if r[0] == name)
    _, bc, _, _, phi_c, phi0_c, vel_c, src_c, nu, dt = _setup(n, dtype, bcname)
    mesh = Mesh(G.box(len(n)), None, list(n), "cuda", dtype)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    _, v_dev = _vels(which, vel_c)
    src = {None: None, "field": src_c.cuda()[0], "scalar": SCALAR_SOURCE}[source]
    return _gpu_launch(mesh, bc, phi_c.cuda(), phi0_c.cuda(), stage, div_kind(limiter, False), v_dev, nu, dt, src)


def test_every_case_runs_on_the_kernel_it_is_meant_for():
    """the launch log (PYAPES_HIP_DEBUG) of one step and one stage per route, in ONE child process"""
    code = ("import torch\nimport test_gpu_velocity as T\n"
            "for r in T.ROUTES:\n"
            "    for stage in (None, (0.75, 0.25)):\n"
            "        torch.cuda.synchronize(); sys.stderr.write('CASE %s %s\\n' % (r[0], 'stage' if stage else 'step')); sys.stderr.flush()\n"
            "        T.route_case(r[0], stage)\n"
            "        torch.cuda.synchronize(); sys.stderr.flush()\n")
    seen = G.case_log(G.child(code), lambda ln: "k_sf" in ln or "k_euler" in ln or "k_cg3d" in ln)
    for name, n, dtype, bcname, limiter, which, source, options, kernel in ROUTES:
        for what in ("step", "stage"):
            lines = seen.get("%s %s" % (name, what))
            assert lines is not None, (name, what, sorted(seen))
            assert len(lines) == 1, (name, what, lines)
            ln = lines[0]
            assert kernel + " " in ln and " (velocity)" in ln and "k_cg3d" not in ln and "k_sfq" not in ln, (name, what, ln)
            periodic_stage = bcname == "xper" and what == "stage"   # the step kernel; k_rk_combine does the stage
            assert ("(RK stage)" in ln) == (what == "stage" and not periodic_stage), (name, what, ln)
            assert ("(source)" in ln) == (source is not None), (name, what, ln)
            if kernel == "k_sf":
                assert " RJ 2" in ln and "kind 4" in ln, ln   # a forced four rows runs the two-row kernel


# ---- switches, march = pieces ---------------------------------------------------------------------------------------
def march_case(n, dtype, bcname, limiter, which, options, order, nsteps, source):
    _, bc, _, _, phi_c, _, vel_c, src_c, nu, dt = _setup(n, dtype, bcname)
    mesh = Mesh(G.box(len(n)), None, list(n), "cuda", dtype)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    f = G.fresh_field(mesh, bc, phi_c)
    _, v_dev = _vels(which, vel_c)
    src = {"field": src_c.cuda(), "scalar": SCALAR_SOURCE, None: None}[source]
    if order == 0:
        euler_march(f, tuple(v_dev), nu, dt, nsteps, G.config(limiter), source=src)
    else:
        rk_march(f, tuple(v_dev), nu, dt, nsteps, G.config(limiter), order=order, source=src)
    return f().clone()


SWITCH_CASES = [([9, 14, 260], "single", "mix", "field"), ([9, 14, 132], "double", "mix", "scalar")]


@pytest.mark.parametrize("n,dtype,bcname,which", SWITCH_CASES, ids=["f32_field", "f64_scalar"])
def test_switches_do_not_change_bits(n, dtype, bcname, which):
    _, _, om, obcs, phi_c, _, vel_c, src_c, nu, dt = _setup(n, dtype, bcname)
    v_ref, _ = _vels(which, vel_c)
    for order, nsteps in ((3, 4), (0, 5)):
        want = R.march(phi_c, v_ref, nu, dt, nsteps, om, obcs, "upwind", max(order, 1), src_c)
        for opts in ({}, {"fastpath": 0}, {"fastpath": 1}, {"sf": 0}, {"sf": 1}, {"sf": 2}, {"sf": 4}, {"chunks": 1}, {"chunks": 2},
                     {"chunks": 3}, {"sf": 4, "chunks": 3}, {"bcl": 0}):
            got = march_case(n, dtype, bcname, "upwind", which, opts, order, nsteps, "field")
            assert bit_equal(got, want), (order, opts, float((got.cpu() - want).abs().max()))


def _march_by_stages(mesh, bc, phi, kind, vel, nu, dt, order, nsteps, source):
    ctx = context_for(mesh)
    f = Field("phi", 1, mesh, bc)
    ctx.bind_bcs(f(), f.bcs, 0)

    def step(phi0):
        out = torch.empty_like(phi0)
        ctx.euler_step_vel(phi0[0], out[0], kind, vel, nu, dt, source=source)
        return out

    def stage(cur, phi0, c0, c1):
        out = torch.empty_like(cur)
        ctx.rk_stage_vel(cur[0], phi0[0], out[0], c0, c1, kind, vel, nu, dt, source=source)
        return out

    return G.march_by_stages(step, stage, phi, order, nsteps)


@pytest.mark.parametrize("limiter", ["upwind", "quick"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_march_is_its_pieces(order, limiter):
    n, dtype, bcname, nsteps = [9, 14, 132], "double", "mix", 3
    mesh, bc, om, obcs, phi_c, _, vel_c, src_c, nu, dt = _setup(n, dtype, bcname)
    kind, cfg = div_kind(limiter, False), G.config(limiter)
    vd = vel_c.cuda()
    for which in ("scalar", "field"):
        v_ref, v_dev = _vels(which, vel_c)
        for source, s_ref in ((None, None), (src_c.cuda()[0], src_c)):
            f = G.fresh_field(mesh, bc, phi_c, time=True)
            g = rk_march(f, tuple(v_dev), nu, dt, nsteps, cfg, order=order, source=source)
            assert g is f
            assert abs(float(f.t) - (1.5 + nsteps * dt)) <= 1e-12          # phi's time advances by nsteps * dt
            pieces = _march_by_stages(mesh, bc, phi_c.cuda(), kind, v_dev, nu, dt, order, nsteps, source)
            assert bit_equal(f(), pieces), (which, float((f() - pieces).abs().max()))
            want = R.march(phi_c, v_ref, nu, dt, nsteps, om, obcs, limiter, order, s_ref)
            assert bit_equal(f(), want), (which, float((f().cpu() - want).abs().max()))
            if order == 1:
                e = euler_march(G.fresh_field(mesh, bc, phi_c), list(v_dev), nu, dt, nsteps, cfg, source=source)
                assert bit_equal(e(), want)
    # the three forms of a velocity give the same bits: the tuple, the (dim, *n) tensor, the vector Field; rk_step too
    want = R.march(phi_c, [vel_c[a] for a in range(3)], nu, dt, nsteps, om, obcs, limiter, order)
    uf = Field("u", 3, mesh, bc)
    uf.set_var_tensor(vd.clone())
    for form in ((vd[0], vd[1], vd[2]), [vd[0], vd[1], vd[2]], vd, uf):
        assert bit_equal(rk_march(G.fresh_field(mesh, bc, phi_c), form, nu, dt, nsteps, cfg, order=order)(), want)
    one = R.march(phi_c, [vel_c[a] for a in range(3)], nu, dt, 1, om, obcs, limiter, order)
    assert bit_equal(rk_step(G.fresh_field(mesh, bc, phi_c), vd, nu, dt, cfg, order=order)(), one)
    # mixed number / tensor entries equal the filled tensors
    mixed = (vd[0], -0.8, vd[2])
    filled = (vd[0], torch.full_like(vd[1], -0.8), vd[2])
    a = rk_march(G.fresh_field(mesh, bc, phi_c), mixed, nu, dt, nsteps, cfg, order=order)()
    b = rk_march(G.fresh_field(mesh, bc, phi_c), filled, nu, dt, nsteps, cfg, order=order)()
    assert bit_equal(a, b)
    assert bit_equal(a, R.march(phi_c, [vel_c[0], -0.8, vel_c[2]], nu, dt, nsteps, om, obcs, limiter, order))


def test_a_c_level_mix_of_scalar_and_field_components():
    """pa_velocity with field[1] == NULL: the generic kernel takes it, and gives the bits of the filled tensor"""
    n, dtype = [9, 14, 132], "double"
    mesh, bc, om, obcs, phi_c, phi0_c, vel_c, src_c, nu, dt = _setup(n, dtype, "mix")
    vd = vel_c.cuda()
    kind = div_kind("upwind", False)
    want = R.euler_step(phi_c, [vel_c[0], -0.8, vel_c[2]], nu, dt, om, obcs, "upwind", src_c)
    got = _gpu_launch(mesh, bc, phi_c.cuda(), phi0_c.cuda(), None, kind, [vd[0], -0.8, vd[2]], nu, dt, src_c.cuda()[0])
    assert bit_equal(got, want)


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_c_abi_errors_leave_the_context_usable():
    n, dtype = [9, 14, 132], "double"
    _, bc, om, obcs, phi_c, phi0_c, vel_c, src_c, nu, dt = _setup(n, dtype, "mix")
    mesh = Mesh(G.box(3), None, list(n), "cuda", dtype)   # a context of its own
    ctx = context_for(mesh)
    f = Field("phi", 1, mesh, bc)
    ctx.bind_bcs(f(), f.bcs, 0)
    lib, h = ctx.lib, ctx.h
    kind = div_kind("upwind", False)
    phi, phi0, src = (t.cuda()[0].contiguous() for t in (phi_c, phi0_c, src_c))
    vd = vel_c.cuda()
    vel = [vd[0], vd[1], vd[2]]
    out, w2 = torch.empty_like(phi), torch.empty_like(phi)
    v_ref = [vel_c[a] for a in range(3)]

    def good():
        ctx.euler_step_vel(phi, out, kind, vel, nu, dt, source=src)
        assert bit_equal(out, R.euler_step(phi_c, v_ref, nu, dt, om, obcs, "upwind", src_c)[0])

    def code_of(call):
        with pytest.raises(PaError) as ei:
            call()
        return ei.value.code

    # vel == NULL, has == 0
    final = C.c_int(-1)
    off = L.PaVelocity()
    off.has = 0
    for v in (None, C.byref(off)):
        assert lib.pa_euler_step_vel(h, G.ptr(phi), G.ptr(out), kind, v, nu, dt, None) == L.PA_E_ARG
        assert lib.pa_rk_stage_vel(h, G.ptr(phi), G.ptr(phi0), G.ptr(out), 0.5, 0.5, kind, v, nu, dt, None) == L.PA_E_ARG
        assert lib.pa_rk_march_vel(h, G.ptr(phi.clone()), G.ptr(out), G.ptr(w2), 3, kind, v, nu, dt, 2, C.byref(final), None) == L.PA_E_ARG
        good()
    # the literal upwind form
    compat = div_kind("upwind", True)
    assert code_of(lambda: ctx.euler_step_vel(phi, out, compat, vel, nu, dt)) == L.PA_E_ARG
    assert code_of(lambda: ctx.rk_stage_vel(phi, phi0, out, 0.5, 0.5, compat, vel, nu, dt)) == L.PA_E_ARG
    assert code_of(lambda: ctx.rk_march_vel(phi.clone(), out, w2, 3, compat, vel, nu, dt, 2)) == L.PA_E_ARG
    good()
    # a velocity field equal to, or overlapping, a buffer of the call or the source field
    p = phi.clone()
    flat = torch.empty(phi.numel() + 16, dtype=phi.dtype, device="cuda")
    base, shifted = flat[:phi.numel()].view(phi.shape), flat[16:].view(phi.shape)   # two views, 128 bytes apart
    for a in range(3):
        def with_(t, a=a):
            return [t if q == a else vel[q] for q in range(3)]
        assert code_of(lambda: ctx.euler_step_vel(phi, out, kind, with_(phi), nu, dt)) == L.PA_E_ARG
        assert code_of(lambda: ctx.euler_step_vel(phi, out, kind, with_(out), nu, dt)) == L.PA_E_ARG
        assert code_of(lambda: ctx.euler_step_vel(phi, out, kind, with_(src), nu, dt, source=src)) == L.PA_E_ARG
        assert code_of(lambda: ctx.euler_step_vel(phi, base, kind, with_(shifted), nu, dt)) == L.PA_E_ARG
        for alias in (phi, phi0, out):
            assert code_of(lambda: ctx.rk_stage_vel(phi, phi0, out, 0.5, 0.5, kind, with_(alias), nu, dt)) == L.PA_E_ARG
        for alias in (p, out, w2):
            assert code_of(lambda: ctx.rk_march_vel(p, out, w2, 3, kind, with_(alias), nu, dt, 2)) == L.PA_E_ARG
        assert code_of(lambda: ctx.rk_march_vel(p, out, None, 1, kind, with_(out), nu, dt, 2)) == L.PA_E_ARG
        assert code_of(lambda: ctx.rk_march_vel(p, out, w2, 2, kind, with_(src), nu, dt, 2, source=src)) == L.PA_E_ARG
    good()
    # a slab context: PA_E_STATE
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    sctx = context_for(slab)
    sphi = torch.zeros(tuple(slab.nx), dtype=torch.float64, device="cuda")
    s1, s2, su = torch.empty_like(sphi), torch.empty_like(sphi), torch.zeros_like(sphi)
    for call in (lambda: sctx.euler_step_vel(sphi, s1, kind, [1.0, 0.5, 0.2], nu, dt),
                 lambda: sctx.rk_stage_vel(sphi, s1, s2, 0.5, 0.5, kind, [su, su.clone(), su.clone()], nu, dt),
                 lambda: sctx.rk_march_vel(sphi, s1, s2, 3, kind, [1.0, 0.5, 0.2], nu, dt, 2)):
        assert code_of(call) == L.PA_E_STATE
    # an axisymmetric mesh: PA_E_ARG
    cyl = Mesh(Cylinder[0:1, 0:1], None, [16, 16], "cuda", "double")
    cctx = context_for(cyl)
    cphi = torch.zeros((16, 16), dtype=torch.float64, device="cuda")
    c1, c2 = torch.empty_like(cphi), torch.empty_like(cphi)
    for call in (lambda: cctx.euler_step_vel(cphi, c1, kind, [1.0, 0.5], nu, dt),
                 lambda: cctx.rk_stage_vel(cphi, c1, c2, 0.5, 0.5, kind, [1.0, 0.5], nu, dt),
                 lambda: cctx.rk_march_vel(cphi, c1, c2, 3, kind, [1.0, 0.5], nu, dt, 2)):
        assert code_of(call) == L.PA_E_ARG
    # the public entry points refuse those meshes before the library is asked
    with pytest.raises(NotImplementedError):
        euler_march(Field("phi", 1, slab, bc), (1.0, 0.5, 0.2), nu, dt, 2)
    with pytest.raises(ValueError):
        euler_step(f, (f()[0], 1.0, 1.0), nu, dt)
    good()
