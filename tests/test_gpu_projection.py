"""-m gpu: the pressure projection -- ``pa_divergence`` / ``pa_project_correct`` (k_divergence, k_project_correct) at the C ABI
and ``divergence`` / ``project`` / ``ns_step`` of pyapes_amd/solver/projection.py.

The yardstick is tests/projection_ref.py, the two kernels restated on the CPU, and the device must give its BITS: three
DISTINCT random components, face values that differ per component, on the smallest meshes where the kernels can go wrong --
whole 16-byte rows and odd ones in 2-D and 3-D, one mesh of two passes of the flat grid, operands off 16-byte alignment with
guards around them -- under all-Dirichlet, mixed Dirichlet / Neumann / symmetry, one periodic axis and fully periodic faces,
in place and out of place, with ``scale`` 1, 1 / dt and negative.  ``project`` is compared with the CPU chain restated kernel ->
oracle CG -> restated kernel at a fixed iteration count, and with the derived fraction of tests/test_projection_host.py on the
converged single-mode problem (the walled one: that module's docstring says why not the periodic one).
"""

import pytest
import torch

import march_gpu as G
import projection_gpu as PG
import projection_ref as PR
import pyapes_oracle as O
from helpers import guards_intact, rel_err, same_bits
from pyapes_amd.geometry import Box, Cylinder
from pyapes_amd.hip import lib as L
from pyapes_amd.hip.context import context_for
from pyapes_amd.hip.lib import PaError
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import FDC
from pyapes_amd.solver.march import momentum_step
from pyapes_amd.solver.projection import divergence, ns_step, project
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

BCS, DT, SCALES, TWO_PASSES = PG.BCS, PG.DT, PG.SCALES, PG.TWO_PASSES
_ids = G.mesh_id


def check_kernels(n, dtype, bcnames, scales=SCALES, offsets=(None,)):
    bad = []
    for bcname in bcnames:
        mesh, bc, om, obcs, U_c, p_c = PG.setup(n, dtype, bcname)[:6]
        ctx = context_for(mesh)
        f = G.fresh_field(mesh, bc, U_c)
        ctx.bind_bcs(f(), f.bcs, 0)
        for scale in scales:
            want_d = PR.divergence(U_c, om, obcs, scale)[0]
            want_c = PR.correct(U_c, p_c, om, obcs, scale)
            want_n = PR.correct(U_c, p_c, om, obcs, scale, fill=False)
            for k in offsets:
                tag = (bcname, scale, k)
                Ud, Ua = PG.dev(U_c, k)
                pd, pa = PG.dev(p_c[0], k)
                dd, da = PG.dev(torch.full_like(p_c[0], float("nan")), k)
                od, oa = PG.dev(torch.full_like(U_c, float("nan")), k)
                got = ctx.divergence(Ud, scale, out=dd)
                if got is not dd or not same_bits(dd, want_d):
                    bad.append((tag, "divergence", same_bits(dd, want_d)))
                got = ctx.project_correct(Ud, pd, scale, f.bcs, out=od)            # out of place: U stays
                if got is not od or not same_bits(od, want_c) or not same_bits(Ud, U_c):
                    bad.append((tag, "out of place", same_bits(od, want_c), same_bits(Ud, U_c)))
                got = ctx.project_correct(Ud, pd, scale, f.bcs)                    # in place, the default
                if got is not Ud or not same_bits(Ud, want_c) or not same_bits(od, Ud):
                    bad.append((tag, "in place", same_bits(Ud, want_c)))
                Ud.copy_(U_c)
                ctx.project_correct(Ud, pd, scale, None)                           # no fill behind the kernel
                if not same_bits(Ud, want_n) or not same_bits(pd, p_c[0]):
                    bad.append((tag, "no fill", same_bits(Ud, want_n)))
                for view, alloc in ((Ud, Ua), (pd, pa), (dd, da), (od, oa)):
                    if alloc is not None and not guards_intact(alloc, view):
                        bad.append((tag, "a guard was written"))
    return bad


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [[9, 132], [11, 13], [10, 12, 132], [11, 13, 17]], ids=_ids)
def test_kernels_give_the_restated_bits(n, dtype):
    assert check_kernels(n, dtype, ("dir", "mix", "xper", "per")) == []


@pytest.mark.parametrize("dtype", ["double", "single"])
def test_kernels_on_two_passes_of_the_flat_grid(dtype):
    """533 628 cells: the second pass of the grid-stride loop covers the last 9 340"""
    assert check_kernels(TWO_PASSES, dtype, ("mix", "per"), scales=(1.0 / DT,)) == []


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [[9, 132], [10, 12, 132], [11, 13, 17]], ids=_ids)
def test_kernels_on_operands_off_16_byte_alignment(n, dtype):
    """every operand 0, 1 (and, fp32, 3) elements past a 16-byte boundary; the sentinels around them stay"""
    offsets = (0, 1) if dtype == "double" else (0, 1, 3)
    assert check_kernels(n, dtype, ("mix", "per"), scales=(-0.75,), offsets=offsets) == []


@pytest.mark.parametrize("n,dtype", [([11, 13], "double"), ([10, 12, 132], "single")], ids=_ids)
def test_divergence_entry_point(n, dtype):
    """``divergence(U)``: the BC fill first (a periodic fill is not idempotent: the reference fills again too), the result
    (1, *n), ``out`` in either shape filled and returned"""
    for bcname in ("mix", "per"):
        mesh, bc, om, obcs, U_c, _ = PG.setup(n, dtype, bcname)[:6]
        filled = O.bc_fill(U_c.clone(), obcs)
        for scale in (1.0, -1.0 / DT):
            want = PR.divergence(filled, om, obcs, scale)
            f = G.fresh_field(mesh, bc, U_c)
            got = divergence(f, scale)
            assert got.shape == (1, *n) and same_bits(got, want) and same_bits(f(), filled), (bcname, scale)
            for shape in ((1, *n), tuple(n)):
                out = torch.full(shape, float("nan"), dtype=U_c.dtype, device="cuda")
                assert divergence(G.fresh_field(mesh, bc, U_c), scale, out) is out
                assert same_bits(out.reshape(want.shape), want)


# ---- composition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", [([11, 13], "double"), ([10, 12, 132], "double"), ([10, 12, 132], "single"), ([11, 13, 17], "single")],
                         ids=_ids)
def test_divergence_is_the_sum_of_the_gradients_diagonal(n, dtype):
    """what a user composed before: ``grad`` of every component, the diagonal summed in torch.  All-Dirichlet faces, where
    Grad's rows are the plain central difference of the filled values (beside neumann / symmetry / periodic faces they are the
    reference's special rows, another operator).  The rounding order differs -- grad forms fl(1 / fl(2 h)) x[+1] + 0 x +
    fl(-1 / fl(2 h)) x[-1] -- so: per axis at most 4 roundings on either side of an operand pair, |difference| <= 8 eps
    (|U[+1]| + |U[-1]|) h_a summed over the axes, cell by cell on the interior set."""
    mesh, bc, om, obcs, U_c, _ = PG.setup(n, dtype, "dir")[:6]
    nd = len(n)
    f = G.fresh_field(mesh, bc, U_c)
    grads = FDC({"grad": {"edge": False}}).grad(f)
    composed = sum(grads[c][c] for c in range(nd)).cpu()
    got = divergence(f)[0].cpu()
    sl = O.interior_slicer(nd, obcs)
    h = [0.5 / float(om.dx[a]) for a in range(nd)]
    bound = sum((torch.roll(U_c[a], -1, a).abs() + torch.roll(U_c[a], 1, a).abs()).double() * h[a] for a in range(nd))
    bound = 8.0 * float(torch.finfo(U_c.dtype).eps) * bound
    diff = (got.double() - composed.double()).abs()
    print(f"composition {n} {dtype}: max difference {float(diff[sl].max()):.3e}, bound there {float(bound[sl].min()):.3e} and up")
    assert bool((diff[sl] <= bound[sl]).all())
    assert float(got[sl].abs().max()) > 1.0


# ---- project --------------------------------------------------------------------------------------------------------
PROJECT_K = 6


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("kind", ["periodic", "walled"])
def test_project_against_the_cpu_chain(kind, dtype):
    """a fixed iteration count (tol -1): U, p and itr against restated divergence -> oracle CG -> restated correction, from a
    non-zero p; the suite's solver tolerances"""
    mesh, om, ubc, pbc, ubcs, pcfg, U_c, p_c = PG.project_case(kind, dtype)
    dt, rho = 0.01, 1.3
    U_w, p_w, rep_w = PR.project(U_c, p_c, dt, rho, om, ubcs, pcfg, -1.0, PROJECT_K)
    Uf, pf = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, p_c)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = project(Uf, pf, dt, rho, {"fdm": {"method": "cg", "tol": -1.0, "max_it": PROJECT_K, "report": False}})
    tol = 1e-10 if dtype == "double" else 1e-5
    eu, ep = rel_err(Uf().cpu(), U_w), rel_err(pf().cpu(), p_w)
    print(f"project {kind} {dtype}: itr {rep['itr']} / {rep_w['itr']}, rel err U {eu:.3e}, p {ep:.3e}")
    assert rep["itr"] == rep_w["itr"] == PROJECT_K + 1
    assert set(rep) == {"itr", "tol", "converge"}
    assert eu <= tol and ep <= tol
    assert rel_err(U_w, U_c) > 1e-3          # the step did something


@pytest.mark.parametrize("dtype", ["double", "single"])
def test_converged_projection_leaves_the_derived_fraction(dtype):
    """the single-mode problem of tests/test_projection_host.py, solved to convergence on the device: the divergence that is
    left, over the divergence before, within 1 % of the constant pinned there"""
    om, U_c, face_vals = PR.mode_case(dtype)
    n = [PR.MODE_N, PR.MODE_N]
    mesh = Mesh(G.box(2), None, n, "cuda", dtype)
    ubc = {"domain": mixed_bcs(face_vals, ["dirichlet"] * 4), "obstacle": None}
    pbc = {"domain": mixed_bcs([0.0] * 4, ["dirichlet"] * 4), "obstacle": None}
    Uf, pf = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, torch.zeros((1, *n), dtype=U_c.dtype))
    before = PR.inner_norm(divergence(Uf).cpu())
    rep = project(Uf, pf, PR.MODE_DT, PR.MODE_RHO, {"fdm": {"method": "cg", "tol": 1e-13 if dtype == "double" else 1e-7,
                                                            "max_it": 500, "report": False}})
    ratio = PR.inner_norm(divergence(Uf).cpu()) / before
    print(f"converged projection {dtype}: itr {rep['itr']}, ratio {ratio!r}, derived {PR.REMAINING_FRACTION!r}")
    assert rep["itr"] < 500
    assert abs(ratio - PR.REMAINING_FRACTION) <= 0.01 * PR.REMAINING_FRACTION


# ---- ns_step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["double", "single"])
def test_ns_step_is_momentum_step_then_project(dtype):
    """bit for bit, and three steps on one context give the bits of a fresh mesh per step"""
    mesh, om, ubc, pbc, ubcs, pcfg, U_c, p_c = PG.project_case("walled", dtype)
    nu, dt, rho = 1e-3, 2e-3, 1.3
    solver = {"fdm": {"method": "cg", "tol": -1.0, "max_it": 4, "report": False}}
    cfg = G.config("upwind")
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Uf, pf = G.fresh_field(mesh, ubc, U_c, time=True), PG.pressure(mesh, pbc, p_c)
        states = []
        for step in range(3):
            rep = ns_step(Uf, pf, nu, dt, cfg, 3, rho=rho, solver=solver)
            assert rep["itr"] == 5
            states.append((Uf().clone(), pf().clone()))
        assert abs(float(Uf.t) - (1.5 + 3 * dt)) <= 1e-12
        # the two halves by hand, on the used mesh
        Ug, pg = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, p_c)
        momentum_step(Ug, nu, dt, cfg, 3)
        project(Ug, pg, dt, rho, solver)
        assert same_bits(Ug(), states[0][0]) and same_bits(pg(), states[0][1])
        # every step again on a mesh that has seen nothing else
        prev = (U_c.cuda(), p_c.cuda())
        for step in range(3):
            fresh = Mesh(G.box(3), None, list(U_c.shape[1:]), "cuda", dtype)
            Uh, ph = G.fresh_field(fresh, ubc, prev[0]), PG.pressure(fresh, pbc, prev[1].clone())
            ns_step(Uh, ph, nu, dt, cfg, 3, rho=rho, solver=solver)
            assert same_bits(Uh(), states[step][0]), (step, same_bits(Uh(), states[step][0]))
            assert same_bits(ph(), states[step][1]), (step, same_bits(ph(), states[step][1]))
            prev = states[step]


# ---- the launch log -------------------------------------------------------------------------------------------------
def log_case():
    mesh, bc, om, obcs, U_c, p_c = PG.setup([11, 13, 17], "double", "mix")[:6]
    f = G.fresh_field(mesh, bc, U_c)
    ctx = context_for(mesh)
    divergence(f)
    ctx.bind_bcs(f(), f.bcs, 0)
    ctx.project_correct(f(), p_c[0].cuda(), 0.5, f.bcs)
    ctx.project_correct(f(), p_c[0].cuda(), 0.5, None, out=torch.empty_like(f()))


def test_the_launches_appear_in_the_launch_log():
    code = ("import torch\nimport test_gpu_projection as T\n"
            "sys.stderr.write('CASE log\\n'); sys.stderr.flush()\n"
            "T.log_case()\ntorch.cuda.synchronize(); sys.stderr.flush()\n")
    lines = G.case_log(G.child(code), lambda ln: "k_divergence" in ln or "k_project_correct" in ln)["log"]
    ncell = 11 * 13 * 17
    assert lines == ["[pyapes_hip] k_divergence: generic kernel, %d cells" % ncell,
                     "[pyapes_hip] k_project_correct (in place): generic kernel, %d cells" % ncell,
                     "[pyapes_hip] k_project_correct: generic kernel, %d cells" % ncell], lines


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_c_abi_errors_leave_the_context_usable():
    n, dtype = [10, 12, 132], "double"
    _, bc, om, obcs, U_c, p_c = PG.setup(n, dtype, "mix")[:6]
    mesh = Mesh(G.box(3), None, list(n), "cuda", dtype)   # a context of its own
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, U_c)
    lib, h = ctx.lib, ctx.h
    ncell = U_c[0].numel()
    want_d = PR.divergence(U_c, om, obcs, 2.0)[0]
    want_c = PR.correct(U_c, p_c, om, obcs, 0.5)
    x = torch.rand(tuple(n), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    want_fill = O.bc_fill(x.clone().unsqueeze(0).repeat(3, 1, 1, 1), obcs)[0]   # component 0's values

    def bound_list_is_component_0s():
        xd = x.cuda()
        ctx.apply_bc_bound(xd)
        assert same_bits(xd, want_fill)

    def good():
        ctx.bind_bcs(f(), f.bcs, 0)
        assert same_bits(ctx.divergence(U_c.cuda(), 2.0), want_d)
        assert same_bits(ctx.project_correct(U_c.cuda(), p_c[0].cuda(), 0.5, f.bcs), want_c)
        bound_list_is_component_0s()       # after a successful call the bound list is what it was

    def code_of(call):
        with pytest.raises(PaError) as ei:
            call()
        return ei.value.code

    good()
    U, p, out, d = U_c.cuda(), p_c[0].cuda(), torch.empty((3, *n), dtype=U_c.dtype, device="cuda"), torch.empty_like(p_c[0]).cuda()
    bv = (L.PaBcValues * 3)()
    for c in range(3):
        bv[c] = ctx.bc_values(f(), f.bcs, c)[0]
    # ncomp != the mesh dimension (the Context always hands mesh.dim: the raw calls)
    for ncomp in (2, 1, 4, 0):
        assert lib.pa_divergence(h, G.ptr(U), ncomp, 1.0, G.ptr(d)) == L.PA_E_ARG
        assert lib.pa_project_correct(h, G.ptr(U), ncomp, G.ptr(p), 1.0, None, bv) == L.PA_E_ARG
    assert lib.pa_divergence(h, None, 3, 1.0, G.ptr(d)) == L.PA_E_ARG
    assert lib.pa_project_correct(h, G.ptr(U), 3, None, 1.0, None, bv) == L.PA_E_ARG
    assert same_bits(U, U_c)
    good()
    # overlapping buffers: the divergence's out on U; p on U or on out; out partly on U
    flat = torch.empty(3 * ncell + 16, dtype=U.dtype, device="cuda")
    base, shifted = flat[:3 * ncell].view(U.shape), flat[16:].view(U.shape)        # two views, 128 bytes apart
    base.copy_(U)
    tail = torch.empty(4 * ncell, dtype=U.dtype, device="cuda")
    lo, hi = tail[:3 * ncell].view(U.shape), tail[ncell:].view(U.shape)            # the last two components on the first two
    for comp in (U[0], U[2], U.reshape(-1)[5:5 + ncell].view(p.shape)):
        assert code_of(lambda: ctx.divergence(U, 1.0, out=comp)) == L.PA_E_ARG
        assert code_of(lambda: ctx.project_correct(U, comp, 1.0, f.bcs)) == L.PA_E_ARG
        assert code_of(lambda: ctx.project_correct(out, comp, 1.0, f.bcs, out=U)) == L.PA_E_ARG
    for a, b in ((base, shifted), (shifted, base), (lo, hi), (hi, lo)):
        assert code_of(lambda: ctx.project_correct(a, p, 1.0, f.bcs, out=b)) == L.PA_E_ARG
    bound_list_is_component_0s()           # after an error the bound list is what it was
    good()
    # a BC face array inside a buffer of the call
    arr_vals = [None if v is None else [v, v, v] for v in BCS["mix"][0]]
    for buf, name in ((U, "U"), (out, "out"), (p, "p")):
        vals = [None if v is None else list(v) for v in arr_vals]
        vals[0][2] = buf.reshape(-1)[7:7 + n[1] * n[2]]                             # face "xl" of component 2
        fb = Field("U", 3, mesh, {"domain": mixed_bcs(vals, BCS["mix"][1]), "obstacle": None})
        assert code_of(lambda: ctx.project_correct(U, p, 1.0, fb.bcs, out=out)) == L.PA_E_ARG, name
    bound_list_is_component_0s()
    good()
    # a live stepwise solve: PA_E_STATE, and after its abort the calls are good again
    var = Field("p", 1, mesh, {"domain": mixed_bcs([0.0] * 6, ["dirichlet"] * 6), "obstacle": None})
    rhs = torch.rand((1, *n), dtype=torch.float64).cuda()
    ctx.bind_bcs(var(), var.bcs, 0)
    ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": 1.0}])
    ctx.cg_begin(var()[0], rhs[0], 1e-30, 1000)
    assert code_of(lambda: ctx.divergence(U, 1.0, out=d)) == L.PA_E_STATE
    assert code_of(lambda: ctx.project_correct(U, p, 1.0, None)) == L.PA_E_STATE
    ctx.cg_abort()
    assert same_bits(U, U_c)
    good()
    # a 1-D mesh, an axisymmetric mesh: PA_E_ARG; a slab: PA_E_STATE
    line = Mesh(G.box(1), None, [33], "cuda", "double")
    l0, l1 = (torch.zeros((1, 33), dtype=torch.float64, device="cuda") for _ in range(2))
    assert code_of(lambda: context_for(line).divergence(l0, 1.0, out=l1[0])) == L.PA_E_ARG
    assert code_of(lambda: context_for(line).project_correct(l0, l1[0], 1.0, None)) == L.PA_E_ARG
    cyl = Mesh(Cylinder[0:1, 0:1], None, [16, 16], "cuda", "double")
    c0, c1 = torch.zeros((2, 16, 16), dtype=torch.float64, device="cuda"), torch.zeros((16, 16), dtype=torch.float64, device="cuda")
    assert code_of(lambda: context_for(cyl).divergence(c0, 1.0, out=c1)) == L.PA_E_ARG
    assert code_of(lambda: context_for(cyl).project_correct(c0, c1, 1.0, None)) == L.PA_E_ARG
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    s0 = torch.zeros((3, *slab.nx), dtype=torch.float64, device="cuda")
    s1 = torch.zeros(tuple(slab.nx), dtype=torch.float64, device="cuda")
    assert code_of(lambda: context_for(slab).divergence(s0, 1.0, out=s1)) == L.PA_E_STATE
    assert code_of(lambda: context_for(slab).project_correct(s0, s1, 1.0, None)) == L.PA_E_STATE
    good()
    # and an ordinary solve on the same context still works
    import warnings
    Uf = G.fresh_field(mesh, bc, U_c)
    pf = PG.pressure(mesh, {"domain": mixed_bcs([0.0] * 6, ["dirichlet"] * 6), "obstacle": None}, torch.zeros_like(p_c))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert project(Uf, pf, 0.01, 1.0, {"fdm": {"method": "cg", "tol": -1.0, "max_it": 2, "report": False}})["itr"] == 3
