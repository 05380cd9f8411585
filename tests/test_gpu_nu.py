"""-m gpu: the diffusivity field of the explicit marches -- ``nu`` a Tensor / Field on the six entry points of
pyapes_amd/solver/march.py, pa_step_nu / pa_march_nu / pa_momentum_march_nu at the C ABI, the NU instantiations of the generic
k_euler and the tiled k_sfn (two marching fields).

The yardstick is tests/march_ref.py, the term div(nu grad phi) and its step restated on the CPU operation for operation, and the
device must give its BITS on every path.  Meshes of the tiled kernel: 14 x 12 x 16 (one partial k tile), 10 x 12 x 132, and
6 x 7 x 260 fp32 / 6 x 7 x 130 fp64 (two k tiles, the second one vector wide; an odd row count at two rows per wave), each with
the chunk cap at 1 and 2, all-dirichlet / mixed / periodic-z / periodic-x faces and u in {0, +0.7, -0.7}.
"""
import ctypes as C

import pytest
import torch

import march_gpu as G
import march_ref as R
import pyapes_oracle as O
from helpers import bit_equal, guards_intact, offset_view
from pyapes_amd.geometry import Box, Cylinder
from pyapes_amd.hip import lib as L
from pyapes_amd.hip.context import context_for
from pyapes_amd.hip.lib import PaError
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.march import euler_march, euler_step, momentum_march, momentum_step, rk_march, rk_step
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

ZPER = G.ZPER
BCS = dict(G.BCS, zper=ZPER)
TILED = [([14, 12, 16], "single"), ([14, 12, 16], "double"), ([10, 12, 132], "single"), ([10, 12, 132], "double"),
         ([6, 7, 260], "single"), ([6, 7, 130], "double")]
STAGE = (0.75, 0.25)

_SETUPS = {}


def setup(n, dtype, bcname):
    """the GPU mesh and BC config, the oracle's mesh and BCs, and CPU tensors from seed 7: two BC-filled fields, a positive
    diffusivity field of mean 1e-3, a speed field, a velocity and a source; dt"""
    key = (tuple(n), dtype, bcname)
    if key not in _SETUPS:
        nd = len(n)
        vals, types = BCS[bcname]
        vals, types = vals[:2 * nd], types[:2 * nd]
        mesh = Mesh(G.box(nd), None, list(n), "cuda", dtype)
        bc = {"domain": mixed_bcs(vals, types), "obstacle": None}
        om = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
        obcs = O.make_bcs(om, O.mixed_cfg(vals, types, O.FACES[:2 * nd]))
        g = torch.Generator().manual_seed(7)
        tdt = mesh.dtype.float
        fields = []
        for _ in range(2):
            t = torch.rand((1, *n), generator=g, dtype=torch.float64).to(tdt)
            O.bc_fill(t, obcs)
            fields.append(t)
        nu = (1e-3 * (0.5 + torch.rand(tuple(n), generator=g, dtype=torch.float64))).to(tdt)
        speed = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        vel = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(tdt)
        src = (3.0 * torch.randn((1, *n), generator=g, dtype=torch.float64)).to(tdt)
        dx = min(float(d) for d in mesh.dx_list)
        dt = 0.2 * min(dx * dx / (2 * nd * 1.5e-3), dx / 1.3)
        _SETUPS[key] = dict(mesh=mesh, bc=bc, om=om, obcs=obcs, phi=fields[0], phi0=fields[1], nu=nu, speed=speed, vel=vel,
                            src=src, dt=dt)
    return _SETUPS[key]


def launch(mesh, bc, phi_d, phi0_d, stage, kind, u, nu_d, dt, source=None):
    """one Euler step (stage None) or stage through the Context (pa_step_nu), the BCs bound; the (1, *n) result"""
    ctx = context_for(mesh)
    f = Field("phi", 1, mesh, bc)
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.full_like(phi_d, float("nan"))
    c0, c1 = stage or (0.0, 0.0)
    ctx.step_nu(phi_d[0], None if stage is None else phi0_d[0], out[0], c0, c1, kind, u, nu_d, dt, source=source)
    return out


def reference(S, stage, u, limiter="upwind", source=None):
    if stage is None:
        return R.euler_step(S["phi"], u, S["nu"], S["dt"], S["om"], S["obcs"], limiter, source)
    return R.rk_stage(S["phi"], S["phi0"], stage[0], stage[1], u, S["nu"], S["dt"], S["om"], S["obcs"], limiter, source)


# ---- the step and the fused stage on the generic and on the tiled kernel ------------------------------------------------
@pytest.mark.parametrize("n,dtype", TILED, ids=G.mesh_id)
def test_step_and_stage_generic_and_tiled(n, dtype):
    bad = []
    for bcname in ("dir", "mix", "zper", "xper"):
        S = setup(n, dtype, bcname)
        ctx = context_for(S["mesh"])
        phi_d, phi0_d, nu_d = S["phi"].cuda(), S["phi0"].cuda(), S["nu"].cuda()
        for u in (0.0, 0.7, -0.7):
            for stage in (None, STAGE):
                want = reference(S, stage, u)
                for opts in ({"sf": 0}, {"sf": 1, "chunks": 1}, {"sf": 1, "chunks": 2}):
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    got = launch(S["mesh"], S["bc"], phi_d, phi0_d, stage, G.kind("upwind"), u, nu_d, S["dt"])
                    if not bit_equal(got, want):
                        bad.append((bcname, u, stage, opts, float((got.cpu() - want).abs().max())))
        ctx.set_option("sf", 1)
        ctx.set_option("chunks", 0)
    assert bad == []


def test_the_field_form_reads_filled_faces_not_the_two_thirds_rows():
    """nu == 1 as a field against nu = 1.0 as a number on the mixed set: the field form reads the FILLED face values where the
    constant form has its Neumann 2/3 rows (they differ by the face's flux value), so the two steps must differ -- the NU path
    cannot silently be the constant one"""
    S = setup([10, 12, 132], "double", "mix")
    ones = torch.ones_like(S["nu"]).cuda()
    got = launch(S["mesh"], S["bc"], S["phi"].cuda(), None, None, G.kind("upwind"), 0.0, ones, 1e-5)
    const = R.euler_step(S["phi"], 0.0, 1.0, 1e-5, S["om"], S["obcs"], "upwind")
    assert bit_equal(got, R.euler_step(S["phi"], 0.0, torch.ones_like(S["nu"]), 1e-5, S["om"], S["obcs"], "upwind"))
    assert not bit_equal(got, const)


# ---- routing ----------------------------------------------------------------------------------------------------------
# name, mesh, dtype, BCs, limiter, speed, options, source, nu placement -> the kernel a step and a stage must run on
ROUTES = [
    ("t_dir_u0_f32", [14, 12, 16], "single", "dir", "upwind", 0.0, {}, False, 0, "k_sfn"),
    ("t_mix_pos_f32", [10, 12, 132], "single", "mix", "upwind", 0.7, {}, False, 0, "k_sfn"),
    ("t_zper_neg_f32", [6, 7, 260], "single", "zper", "upwind", -0.7, {"chunks": 2}, False, 0, "k_sfn"),
    ("t_xper_pos_f32", [10, 12, 132], "single", "xper", "upwind", 0.7, {}, False, 0, "k_sfn"),
    ("t_dir_u0_f64", [14, 12, 16], "double", "dir", "upwind", 0.0, {}, False, 0, "k_sfn"),
    ("t_mix_neg_f64", [10, 12, 132], "double", "mix", "upwind", -0.7, {"chunks": 1}, False, 0, "k_sfn"),
    ("t_zper_pos_f64", [6, 7, 130], "double", "zper", "upwind", 0.7, {}, False, 0, "k_sfn"),
    ("t_xper_u0_f64", [10, 12, 132], "double", "xper", "upwind", 0.0, {}, False, 0, "k_sfn"),
    ("g_sf_off_f32", [10, 12, 132], "single", "mix", "upwind", 0.7, {"sf": 0}, False, 0, "k_euler"),
    ("g_sf_off_f64", [10, 12, 132], "double", "mix", "upwind", 0.7, {"sf": 0}, False, 0, "k_euler"),
    ("g_speed_field_f64", [10, 12, 132], "double", "mix", "upwind", "field", {}, False, 0, "k_euler"),
    ("g_velocity_f32", [10, 12, 132], "single", "mix", "upwind", "velocity", {}, False, 0, "k_euler"),
    ("g_self_f64", [10, 12, 132], "double", "mix", "upwind", "self", {}, False, 0, "k_euler"),
    ("g_quick_f64", [10, 12, 132], "double", "mix", "quick", 0.7, {}, False, 0, "k_euler"),
    ("g_minmod_f32", [10, 12, 132], "single", "mix", "minmod", 0.7, {}, False, 0, "k_euler"),
    ("g_mc_f64", [10, 12, 132], "double", "mix", "mc", -0.7, {}, False, 0, "k_euler"),
    ("g_central_f64", [10, 12, 132], "double", "dir", "none", 0.7, {}, False, 0, "k_euler"),
    ("g_source_f64", [10, 12, 132], "double", "mix", "upwind", 0.7, {}, True, 0, "k_euler"),
    ("g_2d_f64", [17, 12], "double", "mix", "upwind", 0.7, {}, False, 0, "k_euler"),
    ("g_1d_f32", [33], "single", "mix", "upwind", -0.7, {}, False, 0, "k_euler"),
    ("g_odd_rows_f64", [6, 7, 9], "double", "mix", "upwind", 0.7, {}, False, 0, "k_euler"),
    ("g_four_rows_f32", [10, 4, 132], "single", "dir", "upwind", 0.7, {}, False, 0, "k_euler"),
    ("g_unaligned_nu_f32", [10, 12, 132], "single", "mix", "upwind", 0.7, {}, False, 1, "k_euler"),
    ("g_unaligned_nu_f64", [10, 12, 132], "double", "mix", "upwind", 0.0, {}, False, 1, "k_euler"),
]


def route_case(name, stage):
    """one launch of the named route on a fresh mesh (its options are its own); (result, reference, the nu allocation's guards)"""
    _, n, dtype, bcname, limiter, u, options, with_src, shift, _ = next(r for r in ROUTES if r[0] == name)
    S = setup(n, dtype, bcname)
    mesh = Mesh(G.box(len(n)), None, list(n), "cuda", dtype)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    phi_d = S["phi"].cuda()
    nd = len(n)
    if u == "field":
        u_ref, u_dev = S["speed"], S["speed"].cuda()[0]
    elif u == "velocity":
        u_ref, u_dev = [S["vel"][a] for a in range(nd)], [S["vel"].cuda()[a].contiguous() for a in range(nd)]
    elif u == "self":
        u_ref, u_dev = S["phi"], phi_d[0]
    else:
        u_ref = u_dev = u
    nu_d, alloc = offset_view(S["nu"].cuda(), shift)
    src_ref, src_dev = (S["src"], S["src"].cuda()[0]) if with_src else (None, None)
    got = launch(mesh, S["bc"], phi_d, S["phi0"].cuda(), stage, G.kind(limiter), u_dev, nu_d, S["dt"], src_dev)
    return got, reference(S, stage, u_ref, limiter, src_ref), guards_intact(alloc, nu_d)


@pytest.mark.parametrize("name", [r[0] for r in ROUTES if r[-1] == "k_euler"])
def test_every_combination_on_the_generic_kernel(name):
    for stage in (None, STAGE):
        got, want, intact = route_case(name, stage)
        assert bit_equal(got, want), (stage, float((got.cpu() - want).abs().max()))
        assert intact


def test_nu_off_16_byte_alignment_gives_the_same_bits():
    for name in ("t_mix_pos_f32", "t_mix_neg_f64"):
        _, n, dtype, bcname, limiter, u, _, _, _, _ = next(r for r in ROUTES if r[0] == name)
        S = setup(n, dtype, bcname)
        phi_d, phi0_d = S["phi"].cuda(), S["phi0"].cuda()
        for stage in (None, STAGE):
            outs = []
            for shift in (0, 1, 3):
                nu_d, alloc = offset_view(S["nu"].cuda(), shift)
                outs.append(launch(S["mesh"], S["bc"], phi_d, phi0_d, stage, G.kind(limiter), u, nu_d, S["dt"]))
                assert guards_intact(alloc, nu_d)
            assert bit_equal(outs[0], outs[1]) and bit_equal(outs[0], outs[2])
            assert bit_equal(outs[0], reference(S, stage, u))


def test_every_case_runs_on_the_kernel_it_is_meant_for():
    """the launch log (PYAPES_HIP_DEBUG) of one step and one stage per route, in ONE child process; every case prints a marker
    first (the log is limited per kernel instantiation: 8 lines for k_sfn's four, 64 per dtype for the generic kernel)"""
    code = ("import torch\nimport test_gpu_nu as T\n"
            "for r in T.ROUTES:\n"
            "    for stage in (None, T.STAGE):\n"
            "        torch.cuda.synchronize(); sys.stderr.write('CASE %s %s\\n' % (r[0], 'stage' if stage else 'step')); sys.stderr.flush()\n"
            "        T.route_case(r[0], stage)\n"
            "        torch.cuda.synchronize(); sys.stderr.flush()\n")
    seen = G.case_log(G.child(code), lambda ln: "k_sf" in ln or "k_euler" in ln or "k_cg3d" in ln)
    for name, n, dtype, bcname, limiter, u, options, with_src, shift, kernel in ROUTES:
        for what in ("step", "stage"):
            lines = seen.get("%s %s" % (name, what))
            assert lines is not None and len(lines) == 1, (name, what, lines)
            ln = lines[0]
            assert kernel + " " in ln and "(diffusivity field)" in ln, (name, what, ln)
            periodic_stage = bcname in ("xper", "zper") and what == "stage"   # the step kernel; k_rk_combine does the stage
            assert ("(RK stage)" in ln) == (what == "stage" and not periodic_stage), (name, what, ln)
            if kernel == "k_sfn":
                assert " RJ 2" in ln, ln
                if "chunks" in options:
                    assert "chunks %d " % options["chunks"] in ln, ln
            else:
                assert "generic kernel" in ln and ("(source)" in ln) == with_src and ("(velocity)" in ln) == (u == "velocity"), ln


# ---- marches of 3 steps through the public entry points ---------------------------------------------------------------
MARCH_MESHES = [([10, 12, 132], "double"), ([6, 7, 260], "single"), ([6, 7, 9], "double")]


def _nu_forms(S):
    nu_d = S["nu"].cuda()
    fld = Field("nu", 1, S["mesh"], S["bc"])
    fld.set_var_tensor(nu_d.unsqueeze(0).clone())
    return (("component", nu_d), ("field_shaped", nu_d.unsqueeze(0)), ("Field", fld))


@pytest.mark.parametrize("n,dtype", MARCH_MESHES, ids=G.mesh_id)
@pytest.mark.parametrize("order", [1, 2, 3])
def test_rk_march_of_three_steps(n, dtype, order):
    S = setup(n, dtype, "mix")
    want = R.march(S["phi"], 0.7, S["nu"], S["dt"], 3, S["om"], S["obcs"], "upwind", order)
    for form, nu in _nu_forms(S):
        f = G.fresh_field(S["mesh"], S["bc"], S["phi"], time=True)
        g = rk_march(f, 0.7, nu, S["dt"], 3, G.config("upwind"), order=order)
        assert g is f and abs(float(f.t) - (1.5 + 3 * S["dt"])) <= 1e-12
        assert bit_equal(f(), want), (form, float((f().cpu() - want).abs().max()))
    f = G.fresh_field(S["mesh"], S["bc"], S["phi"])
    euler_march(f, 0.7, S["nu"].cuda(), S["dt"], 3, G.config("upwind"))
    assert bit_equal(f(), R.march(S["phi"], 0.7, S["nu"], S["dt"], 3, S["om"], S["obcs"], "upwind", 1))
    if order > 1:   # the single steps
        f = G.fresh_field(S["mesh"], S["bc"], S["phi"])
        for _ in range(3):
            rk_step(f, 0.7, S["nu"].cuda(), S["dt"], G.config("upwind"), order=order)
        assert bit_equal(f(), want)
    else:
        f = G.fresh_field(S["mesh"], S["bc"], S["phi"])
        for _ in range(3):
            euler_step(f, 0.7, S["nu"].cuda(), S["dt"], G.config("upwind"))
        assert bit_equal(f(), want)


COMBOS = ["source", "source_scalar", "velocity_upwind", "velocity_quick", "velocity_numbers", "self", "self_quick", "minmod",
          "mc_field", "central"]


@pytest.mark.parametrize("n,dtype", MARCH_MESHES, ids=G.mesh_id)
@pytest.mark.parametrize("combo", COMBOS)
def test_march_composes_with_every_speed_source_and_limiter(n, dtype, combo):
    S = setup(n, dtype, "dir" if combo == "central" else "mix")
    nd = len(n)
    limiter, u_ref, u_dev, s_ref, s_dev, self_adv = "upwind", 0.7, 0.7, None, None, False
    if combo == "source":
        s_ref, s_dev = S["src"], S["src"].cuda()
    elif combo == "source_scalar":
        s_ref = s_dev = 1.75
    elif combo.startswith("velocity"):
        limiter = "quick" if combo == "velocity_quick" else "upwind"
        if combo == "velocity_numbers":
            u_ref = u_dev = [0.3, -0.2, 0.5][:nd]
        else:
            u_ref, u_dev = [S["vel"][a] for a in range(nd)], S["vel"].cuda()
    elif combo.startswith("self"):
        limiter, self_adv = ("quick" if combo == "self_quick" else "upwind"), True
    elif combo == "minmod":
        limiter = "minmod"
    elif combo == "mc_field":
        limiter, u_ref, u_dev = "mc", S["speed"], S["speed"].cuda()
    elif combo == "central":
        limiter = "none"
    for order in (1, 3):
        f = G.fresh_field(S["mesh"], S["bc"], S["phi"])
        rk_march(f, f if self_adv else u_dev, S["nu"].cuda(), S["dt"], 3, G.config(limiter), order=order, source=s_dev)
        want = R.march(S["phi"], u_ref, S["nu"], S["dt"], 3, S["om"], S["obcs"], limiter, order, s_ref, self_adv=self_adv)
        assert bit_equal(f(), want), (order, float((f().cpu() - want).abs().max()))


@pytest.mark.parametrize("dtype", ["single", "double"])
@pytest.mark.parametrize("frozen", [False, True], ids=["own", "frozen"])
def test_momentum_march_of_three_steps(dtype, frozen):
    n = [8, 9, 16]
    S = setup(n, dtype, "mix")
    tdt = S["mesh"].dtype.float
    g = torch.Generator().manual_seed(9)
    U_c = torch.randn((3, *n), generator=g, dtype=torch.float64).to(tdt)
    for c in range(3):
        O.bc_fill(U_c[c:c + 1], S["obcs"])
    obcs = [S["obcs"]] * 3
    u_ref = [S["vel"][a] for a in range(3)] if frozen else None
    u_dev = S["vel"].cuda() if frozen else None
    for limiter in ("upwind", "quick"):
        for order in (1, 3):
            f = G.fresh_field(S["mesh"], S["bc"], U_c)
            momentum_march(f, S["nu"].cuda(), S["dt"], 3, G.config(limiter), order=order, u=u_dev)
            want = R.momentum.march(U_c, S["nu"], S["dt"], 3, S["om"], obcs, limiter, order, None, u_ref)
            assert bit_equal(f(), want), (limiter, order, float((f().cpu() - want).abs().max()))
    f = G.fresh_field(S["mesh"], S["bc"], U_c)
    momentum_step(f, S["nu"].cuda().unsqueeze(0), S["dt"], G.config("upwind"), order=2, u=u_dev)
    assert bit_equal(f(), R.momentum.march(U_c, S["nu"], S["dt"], 1, S["om"], obcs, "upwind", 2, None, u_ref))


# ---- the generic NU kernel above one pass of its grid -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["single", "double"])
def test_generic_kernel_on_more_cells_than_one_pass_of_its_grid(dtype):
    n = [728, 724]
    assert n[0] * n[1] > 524288
    S = setup(n, dtype, "mix")
    phi_d, phi0_d, nu_d = S["phi"].cuda(), S["phi0"].cuda(), S["nu"].cuda()
    for stage in (None, STAGE):
        got = launch(S["mesh"], S["bc"], phi_d, phi0_d, stage, G.kind("upwind"), -0.7, nu_d, S["dt"], S["src"].cuda()[0])
        want = reference(S, stage, -0.7, "upwind", S["src"])
        assert bit_equal(got, want), (stage, float((got.cpu() - want).abs().max()))


# ---- context reuse ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", [([10, 12, 132], "single"), ([6, 7, 9], "double")], ids=["tiled", "generic"])
def test_constant_field_constant_on_one_mesh_equal_fresh_meshes(n, dtype):
    S = setup(n, dtype, "mix")

    def run(mesh, nu):
        f = G.fresh_field(mesh, S["bc"], S["phi"])
        rk_march(f, 0.7, nu, S["dt"], 3, G.config("upwind"), order=3)
        return f().clone()

    def fresh():
        return Mesh(G.box(3), None, list(n), "cuda", dtype)

    used = fresh()
    nu_d = S["nu"].cuda().clone()
    a = run(used, 1e-3)
    b = run(used, nu_d)
    nu_d.fill_(float("nan"))            # the field's former buffer: nothing of it may be read again
    torch.cuda.synchronize()
    c = run(used, 1e-3)
    b2 = run(used, S["nu"].cuda())
    assert bit_equal(a, run(fresh(), 1e-3)) and bit_equal(c, a)
    assert bit_equal(b, run(fresh(), S["nu"].cuda())) and bit_equal(b2, b)
    assert bit_equal(a, R.march(S["phi"], 0.7, 1e-3, S["dt"], 3, S["om"], S["obcs"], "upwind", 3))
    assert bit_equal(b, R.march(S["phi"], 0.7, S["nu"], S["dt"], 3, S["om"], S["obcs"], "upwind", 3))


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def _dif(t, has=1):
    d = L.PaDiffusivity()
    d.has, d.field = has, (0 if t is None else t.data_ptr())
    return d


def test_has_zero_is_the_sibling():
    """NULL and has == 0 (the field not read): the bits of the sibling entry points, scalar nu used"""
    n, dtype = [10, 12, 132], "double"
    S = setup(n, dtype, "mix")
    mesh = Mesh(G.box(3), None, list(n), "cuda", dtype)
    ctx = context_for(mesh)
    lib, h = ctx.lib, ctx.h
    f = Field("phi", 1, mesh, S["bc"])
    ctx.bind_bcs(f(), f.bcs, 0)
    kind, nu, dt = G.kind("upwind"), 1e-3, S["dt"]
    phi, phi0, uf = (S[k].cuda()[0].contiguous() for k in ("phi", "phi0", "speed"))
    vel = L.PaVelocity()
    vel.has = 1
    for a in range(3):
        vel.value[a] = 0.25 * (a - 1)
    off = _dif(uf, has=0)
    for dif in (None, C.byref(off)):
        a, b = torch.empty_like(phi), torch.empty_like(phi)
        assert lib.pa_euler_step(h, G.ptr(phi), G.ptr(a), kind, 0.9, None, nu, dt) == 0
        assert lib.pa_step_nu(h, G.ptr(phi), None, G.ptr(b), 0.0, 0.0, kind, 0.9, None, None, nu, dt, None, dif) == 0
        assert bit_equal(a, b)
        assert lib.pa_rk_stage(h, G.ptr(phi), G.ptr(phi0), G.ptr(a), 0.75, 0.25, kind, 0.0, G.ptr(uf), nu, dt) == 0
        assert lib.pa_step_nu(h, G.ptr(phi), G.ptr(phi0), G.ptr(b), 0.75, 0.25, kind, 0.0, G.ptr(uf), None, nu, dt, None, dif) == 0
        assert bit_equal(a, b)
        assert lib.pa_euler_step_vel(h, G.ptr(phi), G.ptr(a), kind, C.byref(vel), nu, dt, None) == 0
        assert lib.pa_step_nu(h, G.ptr(phi), None, G.ptr(b), 0.0, 0.0, kind, 0.0, None, C.byref(vel), nu, dt, None, dif) == 0
        assert bit_equal(a, b)
        fa, fb = C.c_int(-1), C.c_int(-1)
        for mode in ("speed", "self", "vel", "euler"):
            bufa = [phi.clone(), torch.empty_like(phi), torch.empty_like(phi)]
            bufb = [phi.clone(), torch.empty_like(phi), torch.empty_like(phi)]
            pa, pb = list(map(G.ptr, bufa)), list(map(G.ptr, bufb))
            if mode == "speed":
                assert lib.pa_rk_march(h, *pa, 3, kind, 0.9, None, nu, dt, 4, C.byref(fa)) == 0
                assert lib.pa_march_nu(h, *pb, 3, kind, 0.9, None, None, 0, nu, dt, 4, C.byref(fb), None, dif) == 0
            elif mode == "self":
                assert lib.pa_rk_march_self(h, *pa, 3, kind, nu, dt, 4, C.byref(fa)) == 0
                assert lib.pa_march_nu(h, *pb, 3, kind, 0.0, None, None, 1, nu, dt, 4, C.byref(fb), None, dif) == 0
            elif mode == "vel":
                assert lib.pa_rk_march_vel(h, *pa, 3, kind, C.byref(vel), nu, dt, 4, C.byref(fa), None) == 0
                assert lib.pa_march_nu(h, *pb, 3, kind, 0.0, None, C.byref(vel), 0, nu, dt, 4, C.byref(fb), None, dif) == 0
            else:
                assert lib.pa_euler_march(h, pa[0], pa[1], kind, -0.8, None, nu, dt, 5) == 0
                fa.value = 1
                assert lib.pa_march_nu(h, pb[0], pb[1], None, 1, kind, -0.8, None, None, 0, nu, dt, 5, C.byref(fb), None, dif) == 0
            assert fa.value == fb.value and bit_equal(bufa[fa.value], bufb[fb.value]), mode


def test_errors_leave_the_context_usable():
    n, dtype = [10, 12, 132], "double"
    S = setup(n, dtype, "mix")
    mesh = Mesh(G.box(3), None, list(n), "cuda", dtype)   # a context of its own
    ctx = context_for(mesh)
    lib, h = ctx.lib, ctx.h
    f = Field("phi", 1, mesh, S["bc"])
    ctx.bind_bcs(f(), f.bcs, 0)
    kind, compat, dt = G.kind("upwind"), G.kind("compat"), S["dt"]
    phi, phi0, nu = (S[k].cuda()[0].contiguous() if S[k].dim() == 4 else S[k].cuda() for k in ("phi", "phi0", "nu"))
    out, w2 = torch.empty_like(phi), torch.empty_like(phi)
    final = C.c_int(-1)

    def step(dif, k=kind, p0=None, o=out):
        return lib.pa_step_nu(h, G.ptr(phi), G.ptr(p0), G.ptr(o), 0.5, 0.5, k, 0.7, None, None, 123.0, dt, None, C.byref(dif))

    def march(dif, k=kind, p=phi, order=3):
        return lib.pa_march_nu(h, G.ptr(p), G.ptr(out), G.ptr(w2), order, k, 0.7, None, None, 0, 123.0, dt, 2, C.byref(final), None,
                               C.byref(dif))

    def good():
        o = torch.empty_like(phi)
        assert step(_dif(nu), o=o) == 0
        assert bit_equal(o, R.euler_step(S["phi"], 0.7, S["nu"], dt, S["om"], S["obcs"], "upwind")[0])   # 123.0 was not read

    good()
    assert step(_dif(None)) == L.PA_E_ARG                       # has != 0 without a field
    for alias in (phi, out):
        assert step(_dif(alias)) == L.PA_E_ARG                  # the field is a buffer of the call
    assert step(_dif(phi0), p0=phi0) == L.PA_E_ARG
    assert step(_dif(phi.view(-1)[8:]), p0=phi0) == L.PA_E_ARG  # or overlaps one
    assert step(_dif(nu), k=compat) == L.PA_E_ARG               # the literal upwind kind
    good()
    p = phi.clone()
    for alias in (p, out, w2):
        assert march(_dif(alias), p=p) == L.PA_E_ARG
    assert march(_dif(None), p=p) == L.PA_E_ARG
    assert march(_dif(nu), k=compat, p=p) == L.PA_E_ARG
    assert march(_dif(nu), p=p, order=4) == L.PA_E_ARG
    assert final.value == -1
    good()
    # the momentum march
    U = torch.randn((3, *n), dtype=torch.float64, device="cuda")
    w1v, w2v = torch.empty_like(U), torch.empty_like(U)
    fU = Field("U", 3, mesh, S["bc"])
    ctx.bind_bcs(fU(), fU.bcs, 0)
    bv = (L.PaBcValues * 3)()
    keep = []
    for q in range(3):
        bv[q], kept = ctx.bc_values(fU(), fU.bcs, q)
        keep.append(kept)
    for alias in (U[1], w1v[2], w2v[0]):
        assert lib.pa_momentum_march_nu(h, G.ptr(U), G.ptr(w1v), G.ptr(w2v), 3, 3, kind, None, 123.0, dt, 2, C.byref(final), None, bv,
                                        C.byref(_dif(alias))) == L.PA_E_ARG
    assert lib.pa_momentum_march_nu(h, G.ptr(U), G.ptr(w1v), G.ptr(w2v), 3, 3, kind, None, 123.0, dt, 2, C.byref(final), None, bv,
                                    C.byref(_dif(None))) == L.PA_E_ARG
    ctx.bind_bcs(f(), f.bcs, 0)
    good()
    # a slab context: PA_E_STATE
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    sctx = context_for(slab)
    sphi = torch.zeros(tuple(slab.nx), dtype=torch.float64, device="cuda")
    s1, s2, snu = torch.empty_like(sphi), torch.empty_like(sphi), torch.ones_like(sphi)
    for call in (lambda: sctx.step_nu(sphi, None, s1, 0.0, 0.0, kind, 1.0, snu, dt),
                 lambda: sctx.step_nu(sphi, s1, s2, 0.5, 0.5, kind, 1.0, snu, dt),
                 lambda: sctx.march_nu(sphi, s1, s2, 3, kind, 1.0, snu, dt, 2)):
        with pytest.raises(PaError) as ei:
            call()
        assert ei.value.code == L.PA_E_STATE, ei.value
    # an axisymmetric mesh: PA_E_ARG
    cyl = Mesh(Cylinder[0:1, 0:1], None, [16, 16], "cuda", "double")
    cctx = context_for(cyl)
    cphi = torch.zeros((16, 16), dtype=torch.float64, device="cuda")
    c1, c2, cnu = torch.empty_like(cphi), torch.empty_like(cphi), torch.ones_like(cphi)
    for call in (lambda: cctx.step_nu(cphi, None, c1, 0.0, 0.0, kind, 1.0, cnu, dt),
                 lambda: cctx.march_nu(cphi, c1, c2, 3, kind, 1.0, cnu, dt, 2)):
        with pytest.raises(PaError) as ei:
            call()
        assert ei.value.code == L.PA_E_ARG, ei.value
    # the public entry points refuse before the library is asked
    with pytest.raises(NotImplementedError):
        euler_march(Field("phi", 1, slab, S["bc"]), 1.0, snu, dt, 2)
    g = G.fresh_field(mesh, S["bc"], S["phi"])
    with pytest.raises(ValueError):
        euler_step(g, 1.0, g()[0], dt)
    # the context that saw the errors still steps, with a field and with a number, and gives the right bits
    good()
    ctx.euler_step(phi, out, kind, 0.9, 1e-3, dt)
    assert bit_equal(out, R.euler_step(S["phi"], 0.9, 1e-3, dt, S["om"], S["obcs"], "upwind")[0])
