"""-m gpu: the source term S of the explicit steps and marches -- ``source=`` of euler_step / euler_march / rk_step / rk_march,
pa_*_src at the C ABI, the SRC instantiations of k_sf and k_sfq and the generic k_euler.

The yardstick is tests/march_ref.py, the step E_S restated on the CPU operation for operation
    a = nu * lap;  a = a - adv;  a = a + s;  a = dt * a;  v = phi + a
and the device must give its BITS: on every kernel path, for the three Div limiters, both signs of a scalar speed, a speed
field, self-advection, Dirichlet and mixed faces, a source field and a scalar source, the Euler step and both fused stages of
order 3.  Meshes: the smallest on which k_sf / k_sfq can still go wrong -- whole 16-byte rows and two k tiles (132 fp64 / 260
fp32 nodes per row), n1 = 13 (a partial row block) and n1 = 14 (what BC on load accepts at two and four rows per wave), n0 =
7 and 9 with the chunk cap at 1, 2 and 3 (every remainder of the chunk length mod 4, one chunk with both faces, uneven
chunks) -- one of n1 = 4 (one row per wave), one with a periodic axis 0 (the unfused stage; k_sfq declines it), and the generic
kernel's: odd rows in 3-D, 2-D, 1-D.  (Smallest for the source term itself; the row-count, row-length and periodic-axis edges of the
kernels -- n1 from 4 to 36, rows of 2 * VEC to 264 nodes, a periodic axis 1 or 2, all-Neumann faces, long chunks under the rule
itself -- are swept for the SRC instantiations in tests/test_gpu_chunks_terms.py.)  The fixed-point test catches a source added in the wrong place, with the wrong sign or
read at the wrong cell: S = -(nu lap - adv)(phi*) makes phi* a fixed point bit for bit.
"""
import ctypes as C

import pytest
import torch

import march_gpu as G
import march_ref as R
import pyapes_oracle as O
from helpers import bit_equal
from march_gpu import GENERIC, VECTOR, VECTOR_OPTIONS
from pyapes_amd.geometry import Box, Cylinder
from pyapes_amd.hip import lib as L
from pyapes_amd.hip.context import context_for
from pyapes_amd.hip.lib import PaError
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.march import SSP_STAGES, euler_march, euler_step, rk_march, rk_step
from pyapes_amd.variables import Field

pytestmark = pytest.mark.gpu

STAGES3 = SSP_STAGES[3]

# scheme: limiter of march_ref, the speed ("field": a random tensor, "self": the field itself), the BC sets it is run with
SCHEMES = {
    "upwind_pos": ("upwind", 0.9, ("dir", "mix")),
    "upwind_neg": ("upwind", -0.8, ("dir", "mix")),
    "upwind_field": ("upwind", "field", ("dir", "mix")),
    "central": ("none", 0.7, ("dir",)),           # central Div refuses neumann / symmetry faces
    "quick_pos": ("quick", 0.9, ("dir", "mix")),
    "quick_neg": ("quick", -0.8, ("dir", "mix")),
    "quick_field": ("quick", "field", ("dir", "mix")),
    "self_upwind": ("upwind", "self", ("dir", "mix")),
    "self_central": ("none", "self", ("dir",)),
    "self_quick": ("quick", "self", ("dir", "mix")),
    "compat": ("compat", 0.7, ("dir", "mix")),     # no SRC instantiation: generic kernel
    "central_field": ("none", "field", ("dir",)),  # a foreign speed at the neighbours: generic kernel
}


def _setup(n, dtype, bcname):
    """march_gpu.setup with ONE speed field: mesh, BC config, oracle mesh and BCs, two BC-filled fields, speed, source, nu, dt"""
    return G.setup(n, dtype, bcname, 1)


def _gpu_launch(mesh, bc, phi_d, phi0_d, stage, kind, u_d, nu, dt, source):
    """one Euler step (stage None) or fused stage through the Context, the BCs bound; returns the (1, *n) result"""
    ctx = context_for(mesh)
    f = Field("phi", 1, mesh, bc)
    ctx.bind_bcs(f(), f.bcs, 0)
    out = torch.full_like(phi_d, float("nan"))
    if stage is None:
        ctx.euler_step(phi_d[0], out[0], kind, u_d, nu, dt, source=source)
    else:
        ctx.rk_stage(phi_d[0], phi0_d[0], out[0], stage[0], stage[1], kind, u_d, nu, dt, source=source)
    return out


def _speeds(u, phi_c, speed_c, phi_d):
    """(the reference's speed, the device's): a float, the speed tensor, or the field itself (the same pointer)"""
    if u == "field":
        return speed_c, speed_c.cuda()[0]
    if u == "self":
        return phi_c, phi_d[0]
    return u, u


SCALAR_SOURCE = 1.75


def run_scheme(n, dtype, scheme, option_sets, bcnames=None):
    limiter, u, scheme_bcs = SCHEMES[scheme]
    bcnames = bcnames or scheme_bcs
    kind = G.kind(limiter)
    bad = []
    for bcname in bcnames:
        mesh, bc, om, obcs, phi_c, phi0_c, speed_c, src_c, nu, dt = _setup(n, dtype, bcname)
        ctx = context_for(mesh)
        phi_d, phi0_d, src_d = phi_c.cuda(), phi0_c.cuda(), src_c.cuda()
        u_ref, u_dev = _speeds(u, phi_c, speed_c, phi_d)
        filled = torch.full_like(src_d, SCALAR_SOURCE)
        for stage in (None, *STAGES3):
            for sname, s_ref, s_dev in (("field", src_c, src_d[0]), ("scalar", SCALAR_SOURCE, SCALAR_SOURCE)):
                if stage is None:
                    want = R.euler_step(phi_c, u_ref, nu, dt, om, obcs, limiter, s_ref)
                else:
                    want = R.rk_stage(phi_c, phi0_c, stage[0], stage[1], u_ref, nu, dt, om, obcs, limiter, s_ref)
                for opts in option_sets:
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    got = _gpu_launch(mesh, bc, phi_d, phi0_d, stage, kind, u_dev, nu, dt, s_dev)
                    if not bit_equal(got, want):
                        bad.append((bcname, stage, sname, opts, float((got.cpu() - want).abs().max())))
                    if sname == "scalar":   # a tensor filled with the scalar: the same bits
                        again = _gpu_launch(mesh, bc, phi_d, phi0_d, stage, kind, u_dev, nu, dt, filled[0])
                        if not bit_equal(got, again):
                            bad.append((bcname, stage, "scalar vs filled tensor", opts))
        ctx.set_option("sf", 1)
        ctx.set_option("chunks", 0)
    return bad


VECTOR_SCHEMES = [s for s in SCHEMES if s not in ("compat", "central_field")]


@pytest.mark.parametrize("scheme", VECTOR_SCHEMES)
@pytest.mark.parametrize("n,dtype", VECTOR, ids=G.mesh_id)
def test_step_and_stage_on_the_vector_kernels(n, dtype, scheme):
    assert run_scheme(n, dtype, scheme, VECTOR_OPTIONS) == []


@pytest.mark.parametrize("scheme", ["upwind_pos", "upwind_field", "central", "self_upwind", "self_central"])
@pytest.mark.parametrize("n,dtype", [([9, 4, 132], "double"), ([9, 4, 260], "single")], ids=["f64", "f32"])
def test_step_and_stage_one_row_per_wave(n, dtype, scheme):
    assert run_scheme(n, dtype, scheme, [{"chunks": 2}]) == []


@pytest.mark.parametrize("scheme", list(SCHEMES))
@pytest.mark.parametrize("n,dtype", GENERIC, ids=G.mesh_id)
def test_step_and_stage_on_the_generic_kernel(n, dtype, scheme):
    assert run_scheme(n, dtype, scheme, [{}]) == []


@pytest.mark.parametrize("scheme", ["compat", "central_field"])
def test_step_and_stage_the_vector_kernels_decline(scheme):
    assert run_scheme([9, 14, 132], "double", scheme, [{}]) == []
    assert run_scheme([9, 14, 260], "single", scheme, [{}]) == []


@pytest.mark.parametrize("scheme", ["upwind_pos", "upwind_field", "central", "quick_neg", "self_upwind", "self_quick"])
def test_step_and_stage_with_a_periodic_axis(scheme):
    """[8, 16, 128] fp32, axis 0 periodic: the stage is the step (with the source), then k_rk_combine, then the fill"""
    assert run_scheme([8, 16, 128], "single", scheme, [{}], bcnames=("xper",)) == []


# ---- routing --------------------------------------------------------------------------------------------------------
# name, mesh, dtype, BCs, scheme, options -> the kernel a step and a stage with a source must run on
ROUTES = [
    ("sf_up_pos_f64", [9, 14, 132], "double", "mix", "upwind_pos", {"sf": 2}, "k_sf"),
    ("sf_up_neg_f32", [9, 14, 260], "single", "mix", "upwind_neg", {"sf": 4}, "k_sf"),
    ("sf_up_field_f32", [7, 13, 260], "single", "dir", "upwind_field", {"sf": 2}, "k_sf"),
    ("sf_central_f64", [7, 13, 132], "double", "dir", "central", {"sf": 4}, "k_sf"),
    ("sf_self_up_f64", [9, 14, 132], "double", "mix", "self_upwind", {"sf": 4}, "k_sf"),
    ("sf_self_central_f32", [9, 14, 260], "single", "dir", "self_central", {"sf": 2}, "k_sf"),
    ("sf_one_row_f64", [9, 4, 132], "double", "dir", "upwind_pos", {}, "k_sf"),
    ("sfq_pos_f32", [9, 14, 260], "single", "mix", "quick_pos", {}, "k_sfq"),
    ("sfq_neg_f64", [7, 13, 132], "double", "dir", "quick_neg", {}, "k_sfq"),
    ("sfq_field_f64", [9, 14, 132], "double", "mix", "quick_field", {}, "k_sfq"),
    ("sfq_self_f32", [7, 13, 260], "single", "mix", "self_quick", {}, "k_sfq"),
    ("sfq_four_rows_asked_f64", [9, 14, 132], "double", "dir", "quick_pos", {"sfq": 4}, "k_sfq"),
    ("gen_compat_f64", [9, 14, 132], "double", "mix", "compat", {}, "k_euler"),
    ("gen_central_field_f32", [9, 14, 260], "single", "dir", "central_field", {}, "k_euler"),
    ("gen_odd_rows_f64", [6, 7, 9], "double", "mix", "upwind_pos", {}, "k_euler"),
    ("gen_2d_f64", [17, 12], "double", "mix", "upwind_neg", {}, "k_euler"),
    ("gen_1d_f32", [33], "single", "mix", "quick_pos", {}, "k_euler"),
    ("gen_sf_off_f64", [9, 14, 132], "double", "mix", "upwind_pos", {"sf": 0}, "k_euler"),
    ("gen_fastpath_off_f32", [9, 14, 260], "single", "mix", "quick_pos", {"fastpath": 0}, "k_euler"),
    ("sf_xper_f32", [8, 16, 128], "single", "xper", "upwind_pos", {}, "k_sf"),
    ("gen_xper_quick_f32", [8, 16, 128], "single", "xper", "quick_pos", {}, "k_euler"),
]


def route_case(name, stage):
    """one launch with a source field of the named route (a fresh mesh, so that its options are its own)"""
    _, n, dtype, bcname, scheme, options, _ = next(r for r in ROUTES if r[0] == name)
    limiter, u, _ = SCHEMES[scheme]
    _, bc, _, _, phi_c, phi0_c, speed_c, src_c, nu, dt = _setup(n, dtype, bcname)
    mesh = Mesh(G.box(len(n)), None, list(n), "cuda", dtype)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    phi_d = phi_c.cuda()
    _, u_dev = _speeds(u, phi_c, speed_c, phi_d)
    return _gpu_launch(mesh, bc, phi_d, phi0_c.cuda(), stage, G.kind(limiter), u_dev, nu, dt, src_c.cuda()[0])


def test_every_case_runs_on_the_kernel_it_is_meant_for():
    """the launch log (PYAPES_HIP_DEBUG) of one step and one stage per route, in ONE child process; the log is limited per
    kernel instantiation, so every case prints a marker first and the routes use distinct instantiations"""
    code = ("import torch\nimport test_gpu_source as T\n"
            "for r in T.ROUTES:\n"
            "    for stage in (None, (0.75, 0.25)):\n"
            "        torch.cuda.synchronize(); sys.stderr.write('CASE %s %s\\n' % (r[0], 'stage' if stage else 'step')); sys.stderr.flush()\n"
            "        T.route_case(r[0], stage)\n"
            "        torch.cuda.synchronize(); sys.stderr.flush()\n")
    seen = G.case_log(G.child(code), lambda ln: "k_sf" in ln or "k_euler" in ln or "k_cg3d" in ln)
    checked = 0
    for name, n, dtype, bcname, scheme, options, kernel in ROUTES:
        for what in ("step", "stage"):
            lines = seen.get("%s %s" % (name, what))
            assert lines is not None, (name, what, sorted(seen))
            if not lines:
                continue   # the instantiation's log budget was used up by an earlier case
            assert len(lines) == 1, (name, what, lines)
            ln = lines[0]
            assert kernel + " " in ln and " (source)" in ln and "k_cg3d" not in ln, (name, what, ln)
            periodic_stage = bcname == "xper" and what == "stage"   # the step kernel; k_rk_combine does the stage
            assert ("(RK stage)" in ln) == (what == "stage" and not periodic_stage), (name, what, ln)
            if kernel == "k_sfq":
                assert " RJ 2" in ln, ln   # option "sfq" = 4 with a source runs two rows
            if name == "sf_one_row_f64":
                assert " RJ 1" in ln, ln
            checked += 1
    assert checked >= len(ROUTES), (checked, seen)
    for name in ("sf_up_pos_f64", "sfq_pos_f32", "gen_compat_f64", "gen_central_field_f32", "gen_odd_rows_f64", "gen_2d_f64"):
        assert seen[name + " step"] and seen[name + " stage"], name


def march_case(n, dtype, bcname, scheme, options, order, nsteps, source):
    limiter, u, _ = SCHEMES[scheme]
    _, bc, _, _, phi_c, _, speed_c, src_c, nu, dt = _setup(n, dtype, bcname)
    mesh = Mesh(G.box(len(n)), None, list(n), "cuda", dtype)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    f = G.fresh_field(mesh, bc, phi_c)
    src = {"field": src_c.cuda(), "scalar": SCALAR_SOURCE, None: None}[source]
    uu = f if u == "self" else (speed_c.cuda() if u == "field" else u)
    if order == 0:
        euler_march(f, uu, nu, dt, nsteps, G.config(limiter), source=src)
    else:
        rk_march(f, uu, nu, dt, nsteps, G.config(limiter), order=order, source=src)
    return f().clone()


def test_a_march_with_a_source_stays_in_the_bc_on_load_form():
    code = ("import torch\nimport test_gpu_source as T\n"
            "sys.stderr.write('CASE a\\n'); sys.stderr.flush()\n"
            "T.march_case([9, 14, 260], 'single', 'mix', 'upwind_pos', {'sf': 4}, 3, 2, 'field'); torch.cuda.synchronize()\n"
            "sys.stderr.write('CASE b\\n'); sys.stderr.flush()\n"
            "T.march_case([9, 14, 132], 'double', 'mix', 'self_upwind', {'sf': 2}, 0, 3, 'scalar'); torch.cuda.synchronize()\n"
            "sys.stderr.write('CASE c\\n'); sys.stderr.flush()\n"
            "T.march_case([9, 14, 132], 'double', 'mix', 'upwind_neg', {'sf': 2, 'bcl': 0}, 3, 1, 'field'); torch.cuda.synchronize()\n")
    seen = G.case_log(G.child(code), lambda ln: "k_sf phase 3" in ln)
    la, lb, lc = seen["a"], seen["b"], seen["c"]
    assert len(la) == 6 and all("(BC on load)" in ln and "(source)" in ln and " RJ 4" in ln for ln in la), la
    assert sum("(RK stage)" in ln for ln in la) == 4, la
    assert len(lb) == 3 and all("(BC on load)" in ln and "(source)" in ln and "(self)" in ln for ln in lb), lb
    assert len(lc) == 3 and all("(source)" in ln and "(BC on load)" not in ln for ln in lc), lc


# ---- switches, march = pieces, no source = today --------------------------------------------------------------------
SWITCH_CASES = [([9, 14, 260], "single", "mix", "upwind_pos"), ([9, 14, 132], "double", "mix", "upwind_field"),
                ([7, 13, 132], "double", "dir", "central"), ([7, 13, 260], "single", "mix", "quick_neg"),
                ([9, 14, 132], "double", "mix", "self_upwind"), ([9, 14, 260], "single", "mix", "self_quick")]


@pytest.mark.parametrize("n,dtype,bcname,scheme", SWITCH_CASES, ids=[c[3] + "_" + c[1] for c in SWITCH_CASES])
def test_switches_do_not_change_bits(n, dtype, bcname, scheme):
    limiter, u, _ = SCHEMES[scheme]
    _, _, om, obcs, phi_c, _, speed_c, src_c, nu, dt = _setup(n, dtype, bcname)
    u_ref = speed_c if u == "field" else (None if u == "self" else u)
    for order, nsteps in ((3, 6), (0, 7)):
        want = R.march(phi_c, u_ref, nu, dt, nsteps, om, obcs, limiter, max(order, 1), src_c, self_adv=u == "self")
        for opts in ({}, {"fastpath": 0}, {"sf": 0}, {"sfq": 0}, {"bcl": 0}, {"chunks": 1}, {"chunks": 2}, {"chunks": 3},
                     {"sf": 2, "chunks": 2}, {"sf": 4, "chunks": 3}):
            got = march_case(n, dtype, bcname, scheme, opts, order, nsteps, "field")
            assert bit_equal(got, want), (order, opts, float((got.cpu() - want).abs().max()))


def _march_by_stages(mesh, bc, phi, kind, u, self_adv, nu, dt, order, nsteps, source):
    ctx = context_for(mesh)
    f = Field("phi", 1, mesh, bc)
    ctx.bind_bcs(f(), f.bcs, 0)

    def step(phi0):
        out = torch.empty_like(phi0)
        ctx.euler_step(phi0[0], out[0], kind, phi0[0] if self_adv else u, nu, dt, source=source)
        return out

    def stage(cur, phi0, c0, c1):
        out = torch.empty_like(cur)
        ctx.rk_stage(cur[0], phi0[0], out[0], c0, c1, kind, cur[0] if self_adv else u, nu, dt, source=source)
        return out

    return G.march_by_stages(step, stage, phi, order, nsteps)


@pytest.mark.parametrize("scheme", ["upwind_pos", "quick_field", "self_upwind", "self_central"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_march_is_its_pieces(order, scheme):
    limiter, u, bcnames = SCHEMES[scheme]
    n, dtype, bcname = [9, 14, 132], "double", bcnames[-1]
    mesh, bc, om, obcs, phi_c, _, speed_c, src_c, nu, dt = _setup(n, dtype, bcname)
    self_adv = u == "self"
    u_dev = speed_c.cuda()[0] if u == "field" else u
    u_ref = speed_c if u == "field" else u
    for source, s_ref in ((src_c.cuda()[0], src_c), (SCALAR_SOURCE, SCALAR_SOURCE)):
        for nsteps in (1, 3):
            f = G.fresh_field(mesh, bc, phi_c)
            uu = f if self_adv else (speed_c.cuda() if u == "field" else u)
            g = rk_march(f, uu, nu, dt, nsteps, G.config(limiter), order=order, source=source)
            assert g is f
            pieces = _march_by_stages(mesh, bc, phi_c.cuda(), G.kind(limiter), u_dev, self_adv, nu, dt, order, nsteps, source)
            assert bit_equal(f(), pieces), (nsteps, float((f() - pieces).abs().max()))
            want = R.march(phi_c, u_ref, nu, dt, nsteps, om, obcs, limiter, order, s_ref, self_adv=self_adv)
            assert bit_equal(f(), want), (nsteps, float((f().cpu() - want).abs().max()))
        f = G.fresh_field(mesh, bc, phi_c)
        uu = f if self_adv else (speed_c.cuda() if u == "field" else u)
        rk_step(f, uu, nu, dt, G.config(limiter), order=order, source=_source_field(mesh, bc, src_c))   # a scalar Field as source
        assert bit_equal(f(), R.march(phi_c, u_ref, nu, dt, 1, om, obcs, limiter, order, src_c, self_adv=self_adv))


def _source_field(mesh, bc, t):
    s = Field("S", 1, mesh, bc)
    s.set_var_tensor(t.cuda())
    return s


def test_source_tensor_forms():
    """one component's shape, a non-contiguous tensor, an int: what euler_step does with them"""
    n, dtype = [9, 14, 132], "double"
    mesh, bc, om, obcs, phi_c, _, _, src_c, nu, dt = _setup(n, dtype, "mix")
    want = R.euler_step(phi_c, 0.9, nu, dt, om, obcs, "upwind", src_c)
    wide = torch.zeros((1, 9, 14, 264), dtype=torch.float64, device="cuda")
    wide[..., ::2] = src_c.cuda()
    for s in (src_c.cuda(), src_c.cuda()[0], wide[..., ::2], wide[0, ..., ::2]):
        f = G.fresh_field(mesh, bc, phi_c)
        assert bit_equal(euler_step(f, 0.9, nu, dt, source=s)(), want)
    f = G.fresh_field(mesh, bc, phi_c)
    assert bit_equal(euler_step(f, 0.9, nu, dt, source=2)(), R.euler_step(phi_c, 0.9, nu, dt, om, obcs, "upwind", 2.0))


@pytest.mark.parametrize("n,dtype", [([9, 14, 260], "single"), ([6, 7, 9], "double")], ids=["vector", "generic"])
def test_no_source_is_today(n, dtype):
    """source=None and the argument left out: the same bits; the five _src entry points with NULL and with has = 0: their
    siblings"""
    mesh, bc, _, _, phi_c, phi0_c, speed_c, _, nu, dt = _setup(n, dtype, "mix")
    cfg = G.config("upwind")

    def fresh():
        return G.fresh_field(mesh, bc, phi_c)

    assert bit_equal(euler_step(fresh(), 0.9, nu, dt, cfg)(), euler_step(fresh(), 0.9, nu, dt, cfg, source=None)())
    assert bit_equal(euler_march(fresh(), 0.9, nu, dt, 5, cfg)(), euler_march(fresh(), 0.9, nu, dt, 5, cfg, source=None)())
    assert bit_equal(rk_step(fresh(), 0.9, nu, dt, cfg)(), rk_step(fresh(), 0.9, nu, dt, cfg, source=None)())
    assert bit_equal(rk_march(fresh(), 0.9, nu, dt, 4, cfg)(), rk_march(fresh(), 0.9, nu, dt, 4, cfg, source=None)())
    f, g = fresh(), fresh()
    assert bit_equal(rk_march(f, f, nu, dt, 4, cfg)(), rk_march(g, g, nu, dt, 4, cfg, source=None)())
    # the C ABI
    ctx = context_for(mesh)
    lib, h = ctx.lib, ctx.h
    ctx.bind_bcs(fresh()(), fresh().bcs, 0)
    kind = G.kind("upwind")
    phi_d, phi0_d, uf = phi_c.cuda()[0].contiguous(), phi0_c.cuda()[0].contiguous(), speed_c.cuda()[0].contiguous()
    off = L.PaSource()
    off.has, off.value, off.field = 0, 123.0, uf.data_ptr()   # has = 0: value and field are not read
    for src in (None, C.byref(off)):
        a, b = torch.empty_like(phi_d), torch.empty_like(phi_d)
        assert lib.pa_euler_step(h, G.ptr(phi_d), G.ptr(a), kind, 0.9, None, nu, dt) == 0
        assert lib.pa_euler_step_src(h, G.ptr(phi_d), G.ptr(b), kind, 0.9, None, nu, dt, src) == 0
        assert bit_equal(a, b)
        assert lib.pa_rk_stage(h, G.ptr(phi_d), G.ptr(phi0_d), G.ptr(a), 0.75, 0.25, kind, 0.0, G.ptr(uf), nu, dt) == 0
        assert lib.pa_rk_stage_src(h, G.ptr(phi_d), G.ptr(phi0_d), G.ptr(b), 0.75, 0.25, kind, 0.0, G.ptr(uf), nu, dt, src) == 0
        assert bit_equal(a, b)
        pa, pb = phi_d.clone(), phi_d.clone()
        assert lib.pa_euler_march(h, G.ptr(pa), G.ptr(a), kind, -0.8, None, nu, dt, 5) == 0
        assert lib.pa_euler_march_src(h, G.ptr(pb), G.ptr(b), kind, -0.8, None, nu, dt, 5, src) == 0
        assert bit_equal(a, b) and bit_equal(pa, pb)
        fa, fb = C.c_int(-1), C.c_int(-1)
        for self_adv in (False, True):
            bufa = [phi_d.clone(), torch.empty_like(phi_d), torch.empty_like(phi_d)]
            bufb = [phi_d.clone(), torch.empty_like(phi_d), torch.empty_like(phi_d)]
            if self_adv:
                assert lib.pa_rk_march_self(h, *map(G.ptr, bufa), 3, kind, nu, dt, 4, C.byref(fa)) == 0
                assert lib.pa_rk_march_self_src(h, *map(G.ptr, bufb), 3, kind, nu, dt, 4, C.byref(fb), src) == 0
            else:
                assert lib.pa_rk_march(h, *map(G.ptr, bufa), 3, kind, 0.9, None, nu, dt, 4, C.byref(fa)) == 0
                assert lib.pa_rk_march_src(h, *map(G.ptr, bufb), 3, kind, 0.9, None, nu, dt, 4, C.byref(fb), src) == 0
            assert fa.value == fb.value and bit_equal(bufa[fa.value], bufb[fb.value])


# ---- fixed point ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["upwind_pos", "central", "quick_neg"])
@pytest.mark.parametrize("n,dtype", [([9, 14, 132], "double"), ([9, 14, 260], "single")], ids=["f64", "f32"])
def test_fixed_point_on_the_gpu(n, dtype, scheme):
    limiter, u, bcnames = SCHEMES[scheme]
    mesh, bc, om, obcs, _, _, _, _, _, _ = _setup(n, dtype, bcnames[-1])
    tdt = mesh.dtype.float
    g = torch.Generator().manual_seed(11)
    star = (torch.rand((1, *n), generator=g, dtype=torch.float64) + 0.5).to(tdt)
    O.bc_fill(star, obcs)
    nu, dt = 0.05, 2e-4
    dx = min(float(d) for d in mesh.dx_list)
    dt = min(dt, 0.1 * dx * dx / (6 * nu))
    S = R.fixed_point_source(star, u, nu, om, obcs, limiter)
    for sf in (2, 4):
        ctx = context_for(mesh)
        ctx.set_option("sf", sf)
        f = G.fresh_field(mesh, bc, star)
        euler_march(f, u, nu, dt, 50, G.config(limiter), source=S.cuda())
        assert torch.equal(f().cpu(), star), float((f().cpu() - star).abs().max())
        f = G.fresh_field(mesh, bc, star)
        rk_march(f, u, nu, dt, 50, G.config(limiter), order=2, source=S.cuda())
        assert torch.equal(f().cpu(), star)
        f = G.fresh_field(mesh, bc, star)
        rk_march(f, u, nu, dt, 50, G.config(limiter), order=3, source=S.cuda())
        dev = float((f().cpu() - star).abs().max())
        ulp = float(torch.finfo(tdt).eps) * float(star.abs().max())
        print(f"{scheme} {dtype} sf {sf}: order 3 max|phi - phi*| = {dev:.3e} ({dev / ulp:.2f} ulp)")
        assert dev <= 4 * ulp, (dev, ulp)
    context_for(mesh).set_option("sf", 1)


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_errors_leave_the_context_usable():
    n, dtype = [9, 14, 132], "double"
    mesh, bc, om, obcs, phi_c, phi0_c, speed_c, src_c, nu, dt = _setup(n, dtype, "mix")
    mesh = Mesh(G.box(3), None, list(n), "cuda", dtype)   # a context of its own
    ctx = context_for(mesh)
    f = Field("phi", 1, mesh, bc)
    ctx.bind_bcs(f(), f.bcs, 0)
    kind = G.kind("upwind")
    phi, phi0, uf, src = (t.cuda()[0].contiguous() for t in (phi_c, phi0_c, speed_c, src_c))
    out, w2 = torch.empty_like(phi), torch.empty_like(phi)

    def arg_error(call):
        with pytest.raises(PaError) as ei:
            call()
        assert ei.value.code == L.PA_E_ARG, ei.value

    # a source aliasing each buffer of a call
    arg_error(lambda: ctx.euler_step(phi, out, kind, uf, nu, dt, source=phi))
    arg_error(lambda: ctx.euler_step(phi, out, kind, uf, nu, dt, source=out))
    arg_error(lambda: ctx.euler_step(phi, out, kind, uf, nu, dt, source=uf))
    arg_error(lambda: ctx.euler_march(phi.clone(), out, kind, uf, nu, dt, 2, source=out))
    p = phi.clone()
    arg_error(lambda: ctx.euler_march(p, out, kind, uf, nu, dt, 2, source=p))
    arg_error(lambda: ctx.euler_march(p, out, kind, uf, nu, dt, 2, source=uf))
    arg_error(lambda: ctx.rk_stage(phi, phi0, out, 0.5, 0.5, kind, uf, nu, dt, source=phi))
    arg_error(lambda: ctx.rk_stage(phi, phi0, out, 0.5, 0.5, kind, uf, nu, dt, source=phi0))
    arg_error(lambda: ctx.rk_stage(phi, phi0, out, 0.5, 0.5, kind, uf, nu, dt, source=out))
    arg_error(lambda: ctx.rk_stage(phi, phi0, out, 0.5, 0.5, kind, uf, nu, dt, source=uf))
    for alias in (p, out, w2, uf):
        arg_error(lambda alias=alias: ctx.rk_march(p, out, w2, 3, kind, uf, nu, dt, 2, source=alias))
    for alias in (p, out, w2):
        arg_error(lambda alias=alias: ctx.rk_march_self(p, out, w2, 3, kind, nu, dt, 2, source=alias))
    arg_error(lambda: ctx.rk_march_self(p, out, None, 1, kind, nu, dt, 2, source=out))
    # a slab context: PA_E_STATE
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    sctx = context_for(slab)
    sphi = torch.zeros(tuple(slab.nx), dtype=torch.float64, device="cuda")
    s1, s2, ssrc = torch.empty_like(sphi), torch.empty_like(sphi), torch.zeros_like(sphi)
    for call in (lambda: sctx.euler_step(sphi, s1, kind, 1.0, nu, dt, source=ssrc),
                 lambda: sctx.euler_march(sphi, s1, kind, 1.0, nu, dt, 2, source=1.0),
                 lambda: sctx.rk_stage(sphi, s1, s2, 0.5, 0.5, kind, 1.0, nu, dt, source=ssrc),
                 lambda: sctx.rk_march(sphi, s1, s2, 3, kind, 1.0, nu, dt, 2, source=1.0),
                 lambda: sctx.rk_march_self(sphi, s1, s2, 3, kind, nu, dt, 2, source=ssrc)):
        with pytest.raises(PaError) as ei:
            call()
        assert ei.value.code == L.PA_E_STATE, ei.value
    # an axisymmetric mesh: PA_E_ARG
    cyl = Mesh(Cylinder[0:1, 0:1], None, [16, 16], "cuda", "double")
    cctx = context_for(cyl)
    cphi = torch.zeros((16, 16), dtype=torch.float64, device="cuda")
    c1, c2, csrc = torch.empty_like(cphi), torch.empty_like(cphi), torch.zeros_like(cphi)
    for call in (lambda: cctx.euler_step(cphi, c1, kind, 1.0, nu, dt, source=csrc),
                 lambda: cctx.euler_march(cphi, c1, kind, 1.0, nu, dt, 2, source=1.0),
                 lambda: cctx.rk_stage(cphi, c1, c2, 0.5, 0.5, kind, 1.0, nu, dt, source=1.0),
                 lambda: cctx.rk_march(cphi, c1, c2, 3, kind, 1.0, nu, dt, 2, source=csrc),
                 lambda: cctx.rk_march_self(cphi, c1, c2, 3, kind, nu, dt, 2, source=1.0)):
        with pytest.raises(PaError) as ei:
            call()
        assert ei.value.code == L.PA_E_ARG, ei.value
    # the public entry points refuse those meshes before the library is asked
    with pytest.raises(NotImplementedError):
        euler_march(Field("phi", 1, slab, bc), 1.0, nu, dt, 2, source=1.0)
    with pytest.raises(ValueError):
        euler_step(f, 1.0, nu, dt, source=f()[0])
    # the context that saw the errors still steps, with and without a source, and gives the right bits
    ctx.euler_step(phi, out, kind, 0.9, nu, dt)
    assert bit_equal(out, R.euler_step(phi_c, 0.9, nu, dt, om, obcs, "upwind")[0])
    ctx.euler_step(phi, out, kind, 0.9, nu, dt, source=src)
    assert bit_equal(out, R.euler_step(phi_c, 0.9, nu, dt, om, obcs, "upwind", src_c)[0])
