"""-m gpu: the momentum march -- ``momentum_step`` / ``momentum_march`` of a vector field that advects itself,
``pa_momentum_march`` at the C ABI, the VEL 3 instantiations of k_sf (upwind, the target's own speed taken from the centre
operand), the aliased VEL 2 instantiations (option ``vself`` 0) and the generic k_euler (everything else).

The yardstick is the momentum functions of tests/march_ref.py, the stage restated on the CPU, and the device must give its
BITS: three DISTINCT random components, face values that DIFFER per component with one component holding a Dirichlet face ARRAY
where the others hold scalars (a swapped component, axis or BC bank cannot pass), no source / a source field per component / a
scalar per component.  Meshes as tests/test_gpu_velocity.py: whole 16-byte rows and two k tiles (132 fp64 / 260 fp32 nodes per
row), n1 = 13 / 14, n0 = 7 / 9 with the chunk cap at 1, 2, 3; the generic kernel's odd rows in 3-D, 2-D; a periodic axis 0.
The exact shift needs no reference.  The frozen form must be d scalar ``rk_march`` calls, the march the stages composed by hand.
"""
import ctypes as C

import pytest
import torch

import march_gpu as G
import march_ref as R
import pyapes_oracle as O
from helpers import bit_equal
from march_gpu import BCS, LIMITER_BCS, VECTOR
from march_ref import momentum as MR
from pyapes_amd.geometry import Box, Cylinder
from pyapes_amd.hip import lib as L
from pyapes_amd.hip.context import context_for
from pyapes_amd.hip.lib import PaError
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import div_kind
from pyapes_amd.solver.march import momentum_march, momentum_step, rk_march
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

ARRAY_FACE, ARRAY_COMP = 3, 1          # face "yu" is dirichlet in every set: component 1 holds an array there
SCALAR_SOURCES = (1.75, -0.5, 0.25)

_ids = G.mesh_id

_SETUPS = {}


def _setup(n, dtype, bcname):
    """the GPU mesh and its BC config (one type per face, a value per component), the oracle mesh and one oracle BC list per
    component, and CPU tensors: a BC-filled vector field with distinct random components, a source per component"""
    key = (tuple(n), dtype, bcname)
    if key not in _SETUPS:
        nd = len(n)
        vals, types = BCS[bcname]
        vals, types = vals[:2 * nd], types[:2 * nd]
        mesh = Mesh(G.box(nd), None, list(n), "cuda", dtype)
        tdt = mesh.dtype.float
        om = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
        g = torch.Generator().manual_seed(5)
        face_n = om.face_mask(O.FACES[ARRAY_FACE]).sum().item()
        arr = torch.randn(face_n, generator=g, dtype=torch.float64).to(tdt)
        per_comp = []                       # per component: the face values, distinct from component to component
        for c in range(nd):
            vc = [None if v is None else v + 0.375 * c - 0.125 * f * c for f, v in enumerate(vals)]
            if c == ARRAY_COMP:
                vc[ARRAY_FACE] = arr
            per_comp.append(vc)
        bc = {"domain": mixed_bcs([None if vals[f] is None else [per_comp[c][f] for c in range(nd)] for f in range(2 * nd)], types),
              "obstacle": None}
        obcs = [O.make_bcs(om, O.mixed_cfg(per_comp[c], types, O.FACES[:2 * nd])) for c in range(nd)]
        U = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(tdt)
        for c in range(nd):
            O.bc_fill(U[c:c + 1], obcs[c])
        src = (3.0 * torch.randn((nd, *n), generator=g, dtype=torch.float64)).to(tdt)
        vel = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(tdt)
        dx = min(float(d) for d in mesh.dx_list)
        nu = 1e-3
        dt = 0.2 * min(dx * dx / (2 * nd * nu), dx / 1.3)
        _SETUPS[key] = (mesh, bc, om, obcs, per_comp, U, src, vel, nu, dt)
    return _SETUPS[key]


def _sources(src_c):
    nd = src_c.shape[0]
    sd = src_c.cuda()
    return ((None, None, None), ("fields", [src_c[c] for c in range(nd)], [sd[c] for c in range(nd)]),
            ("scalars", list(SCALAR_SOURCES[:nd]), list(SCALAR_SOURCES[:nd])))


def run_case(n, dtype, limiter, option_sets, bcnames=None):
    """one Euler step (momentum_step, order 1) and a one-step order-3 march, every source variant, against march_ref.momentum"""
    bad = []
    for bcname in bcnames or LIMITER_BCS[limiter]:
        mesh, bc, om, obcs, _, U_c, src_c, _, nu, dt = _setup(n, dtype, bcname)
        ctx = context_for(mesh)
        for sname, s_ref, s_dev in _sources(src_c):
            want1 = MR.euler_step(U_c, nu, dt, om, obcs, limiter, s_ref)
            want3 = MR.march(U_c, nu, dt, 1, om, obcs, limiter, 3, s_ref)
            for opts in option_sets:
                for k, v in opts.items():
                    ctx.set_option(k, v)
                got1 = momentum_step(G.fresh_field(mesh, bc, U_c), nu, dt, G.config(limiter), order=1, source=s_dev)()
                got3 = momentum_march(G.fresh_field(mesh, bc, U_c), nu, dt, 1, G.config(limiter), order=3, source=s_dev)()
                for what, got, want in (("step", got1, want1), ("march3", got3, want3)):
                    if not bit_equal(got, want):
                        bad.append((bcname, sname, what, opts, float((got.cpu() - want).abs().max())))
        for k, v in (("sf", 1), ("chunks", 0), ("vself", 1)):
            ctx.set_option(k, v)
    return bad


VECTOR_OPTIONS = [{"sf": sf, "chunks": ch, "vself": vs} for sf in (2, 4) for ch in (1, 2, 3) for vs in (0, 1)]


@pytest.mark.parametrize("n,dtype", VECTOR, ids=_ids)
def test_upwind_step_and_march_on_the_vector_kernels(n, dtype):
    assert run_case(n, dtype, "upwind", VECTOR_OPTIONS) == []


@pytest.mark.parametrize("limiter", ["upwind", "quick", "none"])
@pytest.mark.parametrize("n,dtype", [([6, 7, 9], "double"), ([17, 12], "double")], ids=_ids)
def test_step_and_march_on_the_generic_kernel(n, dtype, limiter):
    assert run_case(n, dtype, limiter, [{}]) == []


@pytest.mark.parametrize("limiter", ["upwind", "quick", "none"])
def test_step_and_march_with_a_periodic_axis_0(limiter):
    """the stage is the step, then k_rk_combine, then the fill, per component; the generic kernel"""
    assert run_case([9, 14, 132], "double", limiter, [{}], bcnames=("xper",)) == []


# ---- exact shift ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["single", "double"])
@pytest.mark.parametrize("fastpath", [1, 0], ids=["k_sf", "fastpath0"])
def test_exact_shift(fastpath, dtype):
    """dx = dt = 1, nu = 0, upwind, one Euler step: U_a = +-1 everywhere, the other components small integers that vary along
    axis a only, the faces of the other axes periodic.  U_a stays what it is and the other components move by one node along
    a, exactly.  No reference involved.  (Axis 0 runs k_sf's VEL 3 when the fast path is on; a periodic axis 0 -- a = 1, 2 --
    is the generic kernel's.)"""
    n = [9, 14, 132]
    inner = slice(1, -1)
    for axis in range(3):
        types = ["periodic"] * 6
        types[2 * axis] = types[2 * axis + 1] = "dirichlet"
        for sign in (1.0, -1.0):
            mesh = Mesh(Box[0:8, 0:13, 0:131], None, n, "cuda", dtype)
            assert all(abs(float(d) - 1.0) < 1e-15 for d in mesh.dx_list)
            context_for(mesh).set_option("fastpath", fastpath)
            vals = [None] * 6
            for f in (2 * axis, 2 * axis + 1):
                vals[f] = [sign if c == axis else 2.0 for c in range(3)]
            bc = {"domain": mixed_bcs(vals, types), "obstacle": None}
            g = torch.Generator().manual_seed(7 + axis)
            shape = [n[q] if q == axis else 1 for q in range(3)]
            U = torch.empty((3, *n), dtype=mesh.dtype.float)
            for c in range(3):
                if c == axis:
                    U[c] = sign
                else:
                    ints = torch.randint(-8, 9, (n[axis],), generator=g)
                    ints[ints == 0] = 3                                 # a speed of its own on the other axes: not zero
                    U[c] = ints.to(U.dtype).reshape(shape).expand(*n)
            f = G.fresh_field(mesh, bc, U)
            got = momentum_step(f, 0.0, 1.0, G.config("upwind"), order=1)().cpu()
            sl = tuple(inner if q == axis else slice(None) for q in range(3))
            for c in range(3):
                want = U[c] if c == axis else torch.roll(U[c], 1 if sign > 0 else -1, axis)
                assert torch.equal(got[c][sl], want[sl]), (axis, sign, c)


# ---- the frozen form is d scalar marches ----------------------------------------------------------------------------
def _scalar_bc(per_comp, types, c):
    return {"domain": mixed_bcs(list(per_comp[c]), list(types)), "obstacle": None}


@pytest.mark.parametrize("limiter", ["upwind", "quick"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_frozen_mode_is_one_scalar_march_per_component(order, limiter):
    n, dtype, bcname, nsteps = [9, 14, 132], "double", "mix", 3
    mesh, bc, om, obcs, per_comp, U_c, src_c, vel_c, nu, dt = _setup(n, dtype, bcname)
    types = BCS[bcname][1]
    cfg = G.config(limiter)
    vd = vel_c.cuda()
    for sname, s_ref, s_dev in _sources(src_c)[:2]:
        f = G.fresh_field(mesh, bc, U_c, time=True)
        g = momentum_march(f, nu, dt, nsteps, cfg, order=order, u=vd, source=s_dev)
        assert g is f and abs(float(f.t) - (1.5 + nsteps * dt)) <= 1e-12
        for c in range(3):
            phi = Field("phi", 1, mesh, _scalar_bc(per_comp, types, c))
            phi.set_var_tensor(U_c[c:c + 1].cuda())
            rk_march(phi, (vd[0], vd[1], vd[2]), nu, dt, nsteps, cfg, order=order, source=None if s_dev is None else s_dev[c])
            assert bit_equal(f()[c], phi()[0]), (sname, c, float((f()[c] - phi()[0]).abs().max()))
        want = MR.march(U_c, nu, dt, nsteps, om, obcs, limiter, order, s_ref, u=[vel_c[a] for a in range(3)])
        assert bit_equal(f(), want)
    # the tuple of numbers and the vector Field are the same call
    want = MR.march(U_c, nu, dt, 1, om, obcs, limiter, order, None, u=[0.9, -0.8, 0.4])
    assert bit_equal(momentum_step(G.fresh_field(mesh, bc, U_c), nu, dt, cfg, order=order, u=(0.9, -0.8, 0.4))(), want)


# ---- the march is its pieces ----------------------------------------------------------------------------------------
def _march_by_stages(mesh, f, U, kind, nu, dt, order, nsteps, sources):
    """self mode composed by hand: per stage and component ``bind_bcs(.., c)`` and one pa_*_vel call with CLONES of the stage
    input as the velocity"""
    ctx = context_for(mesh)
    nd = U.shape[0]

    def stage(V, V0, c0, c1):
        frozen = V.clone()
        vel = [frozen[a] for a in range(nd)]
        out = torch.empty_like(V)
        for c in range(nd):
            ctx.bind_bcs(f(), f.bcs, c)
            s = None if sources is None else sources[c]
            if V0 is None:
                ctx.euler_step_vel(V[c], out[c], kind, vel, nu, dt, source=s)
            else:
                ctx.rk_stage_vel(V[c], V0[c], out[c], c0, c1, kind, vel, nu, dt, source=s)
        return out

    return G.march_by_stages(lambda U0: stage(U0, None, None, None), stage, U, order, nsteps)


@pytest.mark.parametrize("order", [2, 3])
@pytest.mark.parametrize("n,dtype,limiter", [([9, 14, 260], "single", "upwind"), ([6, 7, 9], "double", "quick")], ids=["vector", "generic"])
def test_march_is_its_pieces(n, dtype, limiter, order):
    mesh, bc, om, obcs, _, U_c, src_c, _, nu, dt = _setup(n, dtype, "mix")
    kind, cfg, nsteps = div_kind(limiter, False), G.config(limiter), 2
    for sname, s_ref, s_dev in _sources(src_c)[:2]:
        f = G.fresh_field(mesh, bc, U_c)
        momentum_march(f, nu, dt, nsteps, cfg, order=order, source=s_dev)
        pieces = _march_by_stages(mesh, G.fresh_field(mesh, bc, U_c), U_c.cuda(), kind, nu, dt, order, nsteps, s_dev)
        assert bit_equal(f(), pieces), (sname, float((f() - pieces).abs().max()))
        assert bit_equal(f(), MR.march(U_c, nu, dt, nsteps, om, obcs, limiter, order, s_ref))


# ---- routing --------------------------------------------------------------------------------------------------------
# name, mesh, dtype, BCs, limiter, source, options -> kernel, and whether the log names the own axis.  The launch log is limited
# per k_sf instantiation (8 lines): every k_sf route uses instantiations of its own (dtype x VEL x source)
ROUTES = [
    ("vel3_f64", [9, 14, 132], "double", "dir", "upwind", None, {}, "k_sf", True),
    ("vel3_src_f32", [9, 14, 260], "single", "mix", "upwind", "fields", {"chunks": 2}, "k_sf", True),
    ("vel2_f64", [9, 14, 132], "double", "mix", "upwind", None, {"vself": 0}, "k_sf", False),
    ("vel2_src_f32", [7, 13, 260], "single", "dir", "upwind", "scalars", {"vself": 0}, "k_sf", False),
    ("gen_quick_f64", [9, 14, 132], "double", "mix", "quick", None, {}, "k_euler", False),
    ("gen_central_f32", [9, 14, 260], "single", "dir", "none", None, {}, "k_euler", False),
    ("gen_2d_f64", [17, 12], "double", "mix", "upwind", "fields", {}, "k_euler", False),
    ("gen_odd_rows_f64", [6, 7, 9], "double", "mix", "upwind", None, {}, "k_euler", False),
]


def route_case(name):
    """one order-2 step of the named route -- an Euler step and a stage per component -- on a fresh mesh"""
    _, n, dtype, bcname, limiter, source, options, _, _ = next(r for r in ROUTES if r[0] == name)
    _, bc, _, _, _, U_c, src_c, _, nu, dt = _setup(n, dtype, bcname)
    mesh = Mesh(G.box(len(n)), None, list(n), "cuda", dtype)
    for k, v in options.items():
        context_for(mesh).set_option(k, v)
    s_dev = {s[0]: s[2] for s in _sources(src_c)}[source]
    return momentum_step(G.fresh_field(mesh, bc, U_c), nu, dt, G.config(limiter), order=2, source=s_dev)()


def test_every_case_runs_on_the_kernel_it_is_meant_for():
    """the launch log (PYAPES_HIP_DEBUG) of one step and one stage per route, in ONE child process"""
    code = ("import torch\nimport test_gpu_momentum as T\n"
            "for r in T.ROUTES:\n"
            "    torch.cuda.synchronize(); sys.stderr.write('CASE %s\\n' % r[0]); sys.stderr.flush()\n"
            "    T.route_case(r[0])\n"
            "    torch.cuda.synchronize(); sys.stderr.flush()\n")
    seen = G.case_log(G.child(code), lambda ln: "k_sf" in ln or "k_euler" in ln or "k_cg3d" in ln)
    for name, n, dtype, bcname, limiter, source, options, kernel, own in ROUTES:
        nd = len(n)
        lines = seen.get(name)
        assert lines is not None and len(lines) == 2 * nd, (name, lines, sorted(seen))
        for q, ln in enumerate(lines):
            comp, stage = q % nd, q >= nd
            assert kernel + " " in ln and "k_cg3d" not in ln and "k_sfq" not in ln, (name, ln)
            assert ("(RK stage)" in ln) == stage, (name, q, ln)
            assert ("(source)" in ln) == (source is not None), (name, ln)
            if own:
                assert " (velocity, own %d)" % comp in ln, (name, q, ln)
            else:
                assert " (velocity)" in ln, (name, q, ln)
            if kernel == "k_sf":
                assert " RJ 2" in ln and "kind 4" in ln, ln


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_c_abi_errors_leave_the_context_usable():
    n, dtype = [9, 14, 132], "double"
    _, bc, om, obcs, per_comp, U_c, src_c, vel_c, nu, dt = _setup(n, dtype, "mix")
    types = BCS["mix"][1]
    mesh = Mesh(G.box(3), None, list(n), "cuda", dtype)   # a context of its own
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, U_c)
    ctx.bind_bcs(f(), f.bcs, 0)
    lib, h = ctx.lib, ctx.h
    kind = div_kind("upwind", False)
    vd, sd = vel_c.cuda(), src_c.cuda()
    vel, srcs = [vd[a] for a in range(3)], [sd[c] for c in range(3)]
    ncell = U_c[0].numel()

    def bufs():
        return U_c.cuda(), torch.empty((3, *n), dtype=U_c.dtype, device="cuda"), torch.empty((3, *n), dtype=U_c.dtype, device="cuda")

    def good():
        U, w1, w2 = bufs()
        ctx.bind_bcs(f(), f.bcs, 0)
        out = ctx.momentum_march(U, w1, w2, 3, kind, None, nu, dt, 1, srcs, f.bcs)
        assert bit_equal(out, MR.march(U_c, nu, dt, 1, om, obcs, "upwind", 3, [src_c[c] for c in range(3)]))
        # the bound list is what it was: component 0's values (the fill of a scalar shows them)
        x = torch.rand(tuple(n), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        want = O.bc_fill(x.clone().unsqueeze(0), obcs[0])
        xd = x.cuda()
        ctx.apply_bc_bound(xd)
        assert bit_equal(xd, want[0])

    def code_of(call):
        with pytest.raises(PaError) as ei:
            call()
        return ei.value.code

    def march(U, w1, w2, order=3, k=kind, u=None, s=None, bcs=None):
        return ctx.momentum_march(U, w1, w2, order, k, u, nu, dt, 2, s, f.bcs if bcs is None else bcs)

    good()
    U, w1, w2 = bufs()
    # ncomp != the mesh dimension (the Context always hands mesh.dim: the raw call)
    bv = (L.PaBcValues * 3)()
    for c in range(3):
        bv[c] = ctx.bc_values(f(), f.bcs, c)[0]
    final = C.c_int(-1)
    for ncomp in (2, 1, 4):
        assert lib.pa_momentum_march(h, G.ptr(U), G.ptr(w1), G.ptr(w2), ncomp, 3, kind, None, nu, dt, 2, C.byref(final), None, bv) == L.PA_E_ARG
    assert lib.pa_momentum_march(h, G.ptr(U), G.ptr(w1), G.ptr(w2), 3, 4, kind, None, nu, dt, 2, C.byref(final), None, bv) == L.PA_E_ARG
    assert lib.pa_momentum_march(h, G.ptr(U), G.ptr(w1), G.ptr(w2), 3, 3, kind, None, nu, dt, 2, C.byref(final), None, None) == L.PA_E_ARG
    assert final.value == -1
    good()
    # aliased or overlapping buffers
    flat = torch.empty(3 * ncell + 16, dtype=U.dtype, device="cuda")
    base, shifted = flat[:3 * ncell].view(U.shape), flat[16:].view(U.shape)       # two views, 128 bytes apart
    tail = torch.empty(4 * ncell, dtype=U.dtype, device="cuda")
    lo, hi = tail[:3 * ncell].view(U.shape), tail[ncell:].view(U.shape)           # the last two components on the first two
    for a, b, c_ in ((U, U, w2), (U, w1, U), (U, w1, w1), (base, shifted, w2), (U, base, shifted), (lo, w1, hi)):
        assert code_of(lambda: march(a, b, c_)) == L.PA_E_ARG
    assert code_of(lambda: march(U, U, None, order=1)) == L.PA_E_ARG
    assert code_of(lambda: march(base, shifted, None, order=1)) == L.PA_E_ARG
    good()
    # a frozen velocity, a source or a BC face array on a buffer
    for alias in (U[1], w1[0], w2[2]):
        assert code_of(lambda: march(U, w1, w2, u=[vel[0], alias, vel[2]])) == L.PA_E_ARG
        assert code_of(lambda: march(U, w1, w2, s=[None, srcs[1], alias])) == L.PA_E_ARG
    assert code_of(lambda: march(U, w1, None, order=1, u=[w1[0], vel[1], vel[2]])) == L.PA_E_ARG
    face_n = per_comp[ARRAY_COMP][ARRAY_FACE].numel()
    on_buffer = [list(v) for v in per_comp]
    on_buffer[2][0] = w1[1].reshape(-1)[5:5 + n[1] * n[2]]                       # face "xl" of component 2: an array inside w1
    bad_bc = {"domain": mixed_bcs([None if on_buffer[0][q] is None else [on_buffer[c][q] for c in range(3)] for q in range(6)], list(types)),
              "obstacle": None}
    fb = Field("U", 3, mesh, bad_bc)
    assert code_of(lambda: march(U, w1, w2, bcs=fb.bcs)) == L.PA_E_ARG
    assert face_n == n[0] * n[2]
    good()
    # the literal upwind form
    assert code_of(lambda: march(U, w1, w2, k=div_kind("upwind", True))) == L.PA_E_ARG
    good()
    # a 1-D mesh, an axisymmetric mesh: PA_E_ARG; a slab: PA_E_STATE
    line = Mesh(G.box(1), None, [33], "cuda", "double")
    lf = Field("U", 1, line, {"domain": mixed_bcs([0.0, 1.0], ["dirichlet"] * 2), "obstacle": None})
    l0, l1, l2 = (torch.zeros((1, 33), dtype=torch.float64, device="cuda") for _ in range(3))
    assert code_of(lambda: context_for(line).momentum_march(l0, l1, l2, 3, kind, None, nu, dt, 2, None, lf.bcs)) == L.PA_E_ARG
    cyl = Mesh(Cylinder[0:1, 0:1], None, [16, 16], "cuda", "double")
    cf = Field("U", 2, cyl, {"domain": [dict(c, bc_face=fc) for c, fc in zip(mixed_bcs([0.0] * 4, ["dirichlet"] * 4), O.FACES_RZ)],
                             "obstacle": None})
    c0, c1, c2 = (torch.zeros((2, 16, 16), dtype=torch.float64, device="cuda") for _ in range(3))
    assert code_of(lambda: context_for(cyl).momentum_march(c0, c1, c2, 3, kind, None, nu, dt, 2, None, cf.bcs)) == L.PA_E_ARG
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    sf = Field("U", 3, slab, {"domain": mixed_bcs([0.0] * 6, ["dirichlet"] * 6), "obstacle": None})
    s0, s1, s2 = (torch.zeros((3, *slab.nx), dtype=torch.float64, device="cuda") for _ in range(3))
    assert code_of(lambda: context_for(slab).momentum_march(s0, s1, s2, 3, kind, None, nu, dt, 2, None, sf.bcs)) == L.PA_E_STATE
    # the public entry points refuse those before the library is asked
    for field in (lf, cf, sf):
        with pytest.raises(NotImplementedError):
            momentum_march(field, nu, dt, 2)
    good()
    # and a plain scalar march on the same context still gives its reference bits
    phi = Field("phi", 1, mesh, _scalar_bc(per_comp, types, 2))
    phi.set_var_tensor(U_c[2:3].cuda())
    rk_march(phi, (vd[0], vd[1], vd[2]), nu, dt, 2, G.config("upwind"), order=3)
    assert bit_equal(phi(), R.march(U_c[2:3], [vel_c[a] for a in range(3)], nu, dt, 2, om, obcs[2], "upwind", 3))
