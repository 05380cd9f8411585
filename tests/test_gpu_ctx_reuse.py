"""-m gpu: every call on a USED mesh equals the same call on a fresh one.

A mesh owns one ``pa_ctx`` for its whole life, and a program marches, solves, takes gradients and rebinds boundary conditions
on it step after step; the rest of the suite builds a new mesh per run and so only ever sees a context as ``pa_ctx_create``
left it.  The scripts below replay sequences of operations on ONE mesh through tests/reuse_ops.py: every step must equal --
``torch.equal`` on every tensor, ``==`` on ``itr``, ``tol``, every entry of ``ctx.scalars()`` and ``resident_used()`` -- the
same operation on a newly built mesh given the same inputs (the route is the same on both sides, so is the grouping of every
sum: no tolerance).  After each step the caller-owned inputs of the steps behind are overwritten with NaN, so a kernel that
reads a pointer of an earlier binding shows NaN.  The fresh run of each distinct operation is also held against the CPU
references of the suite (oracle/pyapes_oracle.py, tests/march_ref.py) at the suite's bars: bit for bit
for single launches and marches, identical ``itr`` and 1e-10 (fp64) / 1e-5 (fp32) for solver iterates.

What a context remembers, and which call resets it: DESIGN.md, "What a context remembers".
"""
import warnings

import pytest
import torch

import march_gpu as G
import pyapes_oracle as O
import reuse_ops as RO
from reuse_ops import (apply_bcs_op, aop_op, box_mesh, check_gpu_script, failing_solve_op, fdc_op, march_op, option_op, poisson_op,
                       rz_mesh, rz_operators_op, rz_rfp_op, rz_solve_op, solve_op, start_op, stepwise_cg_op)

pytestmark = pytest.mark.gpu


def _rotation(bcname, resident):
    """Jacobi (3 sweeps) -> CG (5) -> BiCGSTAB (4) -> Jacobi (4) -> CG (5) -> Jacobi (3); the repeated CG and Jacobi steps
    must equal their first occurrence as well (reuse_ops.verify: they depend on nothing carried)"""
    want = None if resident is None else bool(resident)
    return [solve_op(m, bcname, k, want_resident=want) for m, k in
            (("jacobi", 3), ("cg", 5), ("bicgstab", 4), ("jacobi", 4), ("cg", 5), ("jacobi", 3))]


# ---- 1. solver rotation, launch per phase -------------------------------------------------------------------------------
ROTATION = {
    "3d_f64_mix": ((20, 37, 50), "double", "mixv", {}),
    "3d_f32_xper_odd_rows": ((12, 18, 133), "single", "xper", {}),       # the pitched CG layout
    "3d_f64_per": ((9, 17, 129), "double", "per", {}),
    "2d_f64": ((40, 44), "double", "mix", {}),
    "2d_f64_cg2d": ((70, 516), "double", "mix", {"cg2d_mincells": 0}),    # k_cg2d forced onto a small mesh (test_gpu_cg2d.py)
}


def _rotation_script(case):
    n, dtype, bcname, opts = ROTATION[case]
    ops = [option_op("resident", 0)] + [option_op(k, v) for k, v in opts.items()] + _rotation(bcname, False)
    return ops, box_mesh(n, dtype)


@pytest.mark.parametrize("case", list(ROTATION), ids=list(ROTATION))
def test_solver_rotation_launch_per_phase(case):
    ops, make = _rotation_script(case)
    steps = check_gpu_script(ops, make)
    assert len(steps) == len(ops)
    assert [s.out["itr"] for s in steps if "itr" in s.out] == [3, 5, 4, 4, 5, 3]


# ---- 2. resident and back -----------------------------------------------------------------------------------------------
RESIDENT = {"3d": ((12, 16, 32), "double"), "2d": ((33, 65), "double"), "1d": ((101,), "double")}


@pytest.mark.parametrize("case", list(RESIDENT), ids=list(RESIDENT))
def test_solver_rotation_resident_and_back(case):
    n, dtype = RESIDENT[case]
    ops = [option_op("resident", 1)] + _rotation("dn", True)
    ops += [option_op("resident", 0), solve_op("cg", "dn", 5, want_resident=False), solve_op("jacobi", "dn", 4, want_resident=False),
            option_op("resident", 1), solve_op("cg", "dn", 5, want_resident=True), solve_op("bicgstab", "dn", 4, want_resident=True)]
    steps = check_gpu_script(ops, box_mesh(n, dtype))
    used = [s.out["resident_used"] for s in steps if "resident_used" in s.out]
    assert all(u > 0 for u in used[:6]) and used[6:8] == [0, 0] and all(u > 0 for u in used[8:]), used


# ---- 3. BC plan rebinding -----------------------------------------------------------------------------------------------
SHUFFLED = [3, 0, 5, 2, 1, 4]
BC_PLANS = [(m, p, r) for m in ("cg", "jacobi") for p, r in ((0, 0), (1, 0), (3, 0), (4, 0), (0, 1), (1, 1), (4, 1))]


@pytest.mark.parametrize("method,bc_path,resident", BC_PLANS, ids=[f"{m}-bc_path{p}-resident{r}" for m, p, r in BC_PLANS])
def test_bc_plan_rebinding(method, bc_path, resident):
    """all-Dirichlet ("no fill after the first") -> mixed -> all-Dirichlet -> periodic -> mixed in shuffled face order, on one
    mesh, with ``Field.apply_bcs`` of another field in between; bc_path 1 / 3 / 4: never the closed form (the pair kernels
    run) / one launch per face / the closed form at any size -- forced the way test_gpu_bc_pair.py and test_gpu_bc_fused.py
    force them.  The oracle comparison of every solve shows that the Neumann and periodic faces were filled."""
    k = 4
    ops = [option_op("resident", resident), option_op("bc_path", bc_path),
           solve_op(method, "dir", k), solve_op(method, "mixv", k), apply_bcs_op("dn"), solve_op(method, "dir", k),
           solve_op(method, "per", k), apply_bcs_op("xper"), solve_op(method, "mixv", k, order=SHUFFLED, seed=8)]
    steps = check_gpu_script(ops, box_mesh((12, 16, 32), "double"))
    used = [s.out["resident_used"] for s in steps if "resident_used" in s.out]
    assert (used[0] > 0) == bool(resident) and (used[1] > 0) == bool(resident), used
    if not resident:
        assert used == [0] * 5


# ---- 4. equation rebinding ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,resident", [((20, 37, 50), 0), ((12, 16, 18), 1)], ids=["launch_per_phase", "resident"])
def test_equation_rebinding(n, resident):
    """scalar-coefficient Laplacian -> tensor-coefficient laplacian(Gamma, .) -> div(u, .) - laplacian with BiCGSTAB and a
    tensor u -> the scalar Laplacian again, ``Aop`` and the rhs adjustment of a third equation between them; Gamma and u of
    the steps behind are poisoned"""
    ops = [option_op("resident", resident),
           solve_op("cg", "dn", 5), aop_op("mix"), solve_op("cg", "dn", 5, eq="gamma"), solve_op("bicgstab", "dn", 4, eq="advdiff"),
           aop_op("mix"), solve_op("cg", "dn", 5), solve_op("jacobi", "dn", 4, eq="gamma"), solve_op("cg", "dn", 5)]
    check_gpu_script(ops, box_mesh(n, "double"))


# ---- 5. a time loop -----------------------------------------------------------------------------------------------------
LOOP = {"f32_whole_rows": ((12, 20, 136), "single"),      # whole 16-byte rows: k_sf's VEL instantiations, k_sfq
        "f64_generic": ((11, 13, 17), "double")}          # the generic kernels


def _cycle():
    return [march_op("momentum"), march_op("quick3"), march_op("minmod2"), march_op("euler"), march_op("self"), poisson_op(5),
            fdc_op("grad"), fdc_op("laplacian")]


@pytest.mark.parametrize("case", list(LOOP), ids=list(LOOP))
def test_time_loop(case):
    """three cycles of momentum_march, rk_march (order 3 quick; order 2 minmod with a source), euler_march (bcl 1),
    rk_march(phi, phi), a CG Poisson solve, FDC.grad and FDC.laplacian, the fields carried from step to step; every step
    against a fresh mesh given the carried tensors, and against tests/march_ref.py / the oracle"""
    n, dtype = LOOP[case]
    ops = [start_op()] + _cycle() * 3
    steps = check_gpu_script(ops, box_mesh(n, dtype))
    assert len(steps) == 25
    assert all(bool(torch.isfinite(v).all()) for s in steps for v in s.out.values() if isinstance(v, torch.Tensor))


# ---- 6. option round trips ------------------------------------------------------------------------------------------------
OPTION_TRIPS = [("chunks", 3, 0), ("sf", 2, 1), ("sfq", 0, 1), ("fold", 0, 1), ("fastpath", 0, 1), ("bcl", 0, 1)]


@pytest.mark.parametrize("case", list(LOOP), ids=list(LOOP))
def test_option_round_trips(case):
    """on one context, one option after another set and put back: every result equals a fresh context created with the
    options in force, and after the last restore a fresh default context"""
    n, dtype = LOOP[case]

    def body():      # the single-field operations of the rotation and of the time loop, all of them
        return [solve_op("cg", "mixv", 5), solve_op("jacobi", "mixv", 4), solve_op("bicgstab", "mixv", 4)] + _cycle()
    ops = [option_op("resident", 0), start_op()]
    for name, value, default in OPTION_TRIPS:
        ops += [option_op(name, value)] + body() + [option_op(name, default)]
    ops += body()
    steps = check_gpu_script(ops, box_mesh(n, dtype))
    assert steps[-1].before.options == {"resident": 0, **{name: default for name, _, default in OPTION_TRIPS}}


def test_set_option_during_a_live_stepwise_solve_stays_refused():
    from pyapes_amd.hip import lib as L
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.variables import Field
    make = box_mesh((20, 37, 50), "double")
    mesh = make()
    ctx = context_for(mesh)
    cfg, _, _ = RO.bc_configs(mesh, RO.BCSETS["mix"], None, 0)
    var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
    rhs = RO._rand(mesh, 7).cuda()
    ctx.bind_bcs(var(), var.bcs, 0)
    ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": 0.7}])
    ctx.cg_begin(var()[0], rhs[0], 1e-30, 1000)
    try:
        ctx.cg_iterate(2)
        before = ctx.get_option("fold")
        with pytest.raises(RuntimeError, match="pa_ctx_set_option during a solve"):
            ctx.set_option("fold", 0)
        assert ctx.get_option("fold") == before
    finally:
        ctx.cg_abort()
    ctx.set_option("fold", 0)       # accepted again once the solve is gone
    ctx.set_option("fold", before)
    op = solve_op("cg", "mixv", 5)
    got = op(mesh, RO.Carried())
    # (the poisoning of dropped bindings reads HipContext._keep: after a solve with a face-value array it is not empty)
    assert len(RO.held_by_context(mesh)) >= 1
    assert RO.differences(got, RO.run_fresh(op, RO.Carried(), make)) == []


# ---- 7. interrupted and failed solves -----------------------------------------------------------------------------------
def _keep_old_op():
    """``save_old`` True, then False: after the second solve the buffer that used to be VARo, filled with a sentinel, is
    untouched -- ``pa_solver_keep_old(None)`` has taken effect"""
    def fn(mesh, carried):
        from pyapes_amd.solver.fdm import FDM
        from pyapes_amd.solver.ops import Solver
        from pyapes_amd.variables import Field
        cfg, _, arrays = RO.bc_configs(mesh, RO.BCSETS["mix"], None, 0)
        out = {}
        old = None
        for tag, save in (("kept", True), ("plain", False)):
            var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
            rhs = RO._rand(mesh, 7).cuda()
            s = Solver({"fdm": {"method": "cg", "tol": -1.0, "max_it": 3, "report": False, "save_old": save}})
            s.set_eq(-FDM().laplacian(0.7, var) == rhs)
            rep = RO._quiet(s.solve)
            out[tag] = {"x": var().cpu(), **RO._report(mesh, rep)}
            if save:
                old = var.VARo
                out["x_old"] = old.cpu()
                old.fill_(G_SENTINEL)
            carried.own(var(), rhs)
        out["old_untouched"] = bool((old == G_SENTINEL).all())
        carried.own(old, *arrays)
        return out

    def ref(before, out, mesh):
        assert out["old_untouched"] is True
        assert torch.equal(out["kept"]["x"], out["plain"]["x"]) and out["kept"]["tol"] == out["plain"]["tol"]
        _, ocfg, _ = RO.bc_configs(mesh, RO.BCSETS["mix"], None, 0)
        for k, got in ((3, out["kept"]["x"]), (2, out["x_old"])):      # VARo: the iterate one iteration earlier
            xo, ro = RO._quiet(lambda: O.solve_poisson(RO._omesh(mesh), ocfg, RO._rand(mesh, 7), method="cg", tol=-1.0, max_it=k,
                                                       coeff=0.7, sign=-1.0))
            assert ro["itr"] == k + 1 and (k == 2 or out["kept"]["itr"] == ro["itr"])
            assert RO._rel(got, xo) < 1e-10, (k, RO._rel(got, xo))

    return RO.Op("save_old-then-not", fn, ref, pure=True)


G_SENTINEL = -123456.789


def test_interrupted_and_failed_solves():
    ops = [option_op("resident", 0),
           stepwise_cg_op("mix", 2, finish=False), solve_op("cg", "mix", 5), solve_op("jacobi", "mix", 4), solve_op("bicgstab", "mix", 4),
           stepwise_cg_op("mix", 3, finish=True), solve_op("jacobi", "mix", 3),
           failing_solve_op("cg"), solve_op("cg", "mix", 5), failing_solve_op("jacobi"), solve_op("jacobi", "mix", 4),
           failing_solve_op("bicgstab"), solve_op("bicgstab", "mix", 4),
           _keep_old_op(), solve_op("cg", "mix", 5), stepwise_cg_op("mix", 3, finish=True)]
    check_gpu_script(ops, box_mesh((20, 37, 50), "double"))


def test_failed_solve_on_the_resident_path_then_a_good_one():
    ops = [option_op("resident", 1), solve_op("cg", "dn", 5, want_resident=True), failing_solve_op("cg"),
           solve_op("cg", "dn", 5, want_resident=True), failing_solve_op("jacobi"), solve_op("jacobi", "dn", 4, want_resident=True),
           _keep_old_op(), solve_op("bicgstab", "dn", 4, want_resident=True)]
    check_gpu_script(ops, box_mesh((12, 16, 32), "double"))


# ---- 8. stepwise Jacobi parity ------------------------------------------------------------------------------------------
# A sweep over ONE plane sums the same way in either direction, and a mesh of (24, 20, 132) gets one chunk per plane by the
# kernel's own rule: "chunks" 1 makes every workgroup march over all planes, as the meshes of real runs do.  Measured on the
# parent of the commit that added this test (no reset of the sweep direction), (48, 40, 132) fp64, chunks 1, a first solve of
# 5 sweep launches, then 7: tol 0.20354028997991275 on the used mesh, 0.20354028997991272 on a fresh one.
PARITY_JOBS = {
    "24x20x132_jac_alt1": ((24, 20, 132), {"jac_alt": 1}), "24x20x132_jac_alt0": ((24, 20, 132), {"jac_alt": 0}),
    "24x20x132_chunks1_jac_alt1": ((24, 20, 132), {"jac_alt": 1, "chunks": 1}),
    "48x40x132_chunks1_jac_alt1": ((48, 40, 132), {"jac_alt": 1, "chunks": 1}),
    "48x40x132_chunks1_jac_alt0": ((48, 40, 132), {"jac_alt": 0, "chunks": 1}),      # the control
}
_PARITY_ORACLE = {}


@pytest.fixture(scope="module")
def jacobi_parity(tmp_path_factory):
    """ONE spawned rank process (the gloo group of tests/test_gpu_slab.py) runs every job"""
    from test_slab_gloo import spawn_ranks
    jobs = [(key, n, "double", opts, 4, 6) for key, (n, opts) in PARITY_JOBS.items()]
    out = str(tmp_path_factory.mktemp("jacobi_parity") / "res.pt")
    spawn_ranks(RO.jacobi_parity_worker, lambda port: (1, port, jobs, out), 1)
    return torch.load(out)


@pytest.mark.parametrize("key", list(PARITY_JOBS))
def test_stepwise_jacobi_after_an_odd_number_of_sweep_launches(key, jacobi_parity):
    """two SlabJacobi solves on one mesh, the first with 5 sweep launches: the second must report exactly the ``itr``, the
    ``tol`` (and the stop-test sum under it, and the iterate) of the same solve on a fresh mesh.  The direction of the next
    sweep (``jac_dir``) used to survive the solve, so with alternating sweeps (``jac_alt`` 1) the second solve summed its stop
    test in the other order; ``jac_alt`` 0 is the control, where it always held."""
    n = PARITY_JOBS[key][0]
    res = jacobi_parity[key]
    first, second, fresh = res["first"], res["second"], res["fresh"]
    assert first["itr"] == 5 and fresh["itr"] == 7
    if n not in _PARITY_ORACLE:
        om = O.OMesh([0, 0, 0], [1, 1, 0.5], list(n), "double")
        cfg = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(RO.BCSETS["mix"])]
        rhs = torch.randn((1, *n), generator=torch.Generator().manual_seed(8), dtype=torch.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _PARITY_ORACLE[n] = O.solve_poisson(om, cfg, rhs, method="jacobi", tol=1e-30, max_it=6, coeff=0.7, sign=-1.0, omega=0.9)
    xo, ro = _PARITY_ORACLE[n]
    assert ro["itr"] == fresh["itr"] and RO._rel(fresh["x"], xo) < 1e-10
    assert second["itr"] == fresh["itr"]
    assert second["tol"] == fresh["tol"], (second["tol"], fresh["tol"])
    assert second["dx2"] == fresh["dx2"], (second["dx2"], fresh["dx2"])
    assert torch.equal(second["x"], fresh["x"])


# ---- 9. axisymmetric mesh -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [(21, 21), (33, 65)], ids=["21x21", "33x65"])
def test_axisymmetric_mesh(n, dtype):
    """the operators that read the r table of ``pa_coord_set`` (a scratch slot of the context), a BiCGSTAB solve that has to
    allocate its own scratch slots beside it, the operators again, the Fokker-Planck operators, a Jacobi solve, the
    operators once more"""
    ops = [rz_operators_op(), rz_solve_op("bicgstab", 5), rz_operators_op(), rz_rfp_op(), rz_solve_op("jacobi", 4), rz_solve_op("cg", 5),
           rz_operators_op(), rz_rfp_op()]
    check_gpu_script(ops, rz_mesh(n, dtype))


# ---- the paths the scripts exist to reach -------------------------------------------------------------------------------
def paths_child():
    """(child process, launch log on) the script side of three scripts, a marker in front of each"""
    import sys
    warnings.simplefilter("ignore")
    for name, (ops, make) in (("pitched", _rotation_script("3d_f32_xper_odd_rows")), ("cg2d", _rotation_script("2d_f64_cg2d")),
                              ("loop", ([start_op()] + _cycle(), box_mesh(*LOOP["f32_whole_rows"])))):
        print("CASE " + name, file=sys.stderr, flush=True)
        RO.run_script(ops, make)
        torch.cuda.synchronize()


def test_the_scripts_reach_their_paths():
    """the launch log (PYAPES_HIP_DEBUG) of the scripts' own runs, in ONE child process: odd fp32 rows run the pitched CG
    phases, the forced 2-D mesh k_cg2d, the whole-row fp32 time loop k_sf's velocity instantiations and k_sfq.  (The resident
    launches are shown by ``resident_used`` in the scripts themselves, the BC-fill kernels by the ``bc_path`` bits.)"""
    log = G.child("import test_gpu_ctx_reuse as T\nT.paths_child()\n", drop_options=True)
    seen = G.case_log(log, lambda ln: ln.startswith("[pyapes_hip]"))
    pitched, cg2d, loop = ("\n".join(seen[k]) for k in ("pitched", "cg2d", "loop"))
    assert "k_cg3d phase A (pitched)" in pitched and "k_cg3d phase B (pitched)" in pitched, pitched
    assert "k_cg2d phase A" in cg2d and "k_cg2d phase B" in cg2d, cg2d
    assert "k_sf phase" in loop and "(velocity, own" in loop and "k_sfq phase 3" in loop, loop
    assert "(BC on load)" in loop, loop


# ---- vec_axpy with its output aliased ---------------------------------------------------------------------------------------
# more cells than ONE pass of the grid covers: pa_grid_blocks caps a grid at 2048 blocks of 256 threads = 524288 cells
AXPY_MESHES = {"7x9x11": (7, 9, 11), "17x128x243": (17, 128, 243)}


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("mesh_id", list(AXPY_MESHES))
def test_vec_axpy_out_may_alias_its_inputs(mesh_id, dtype):
    """``vec_axpy(out, y, a, x)``: out = y + a * x, the product rounded first, no FMA -- with ``out is y``, ``out is x`` and
    all three the same tensor (what solver/host_stepped.py calls), bit for bit against the CPU statement"""
    from pyapes_amd.hip.context import context_for
    n = AXPY_MESHES[mesh_id]
    assert (n[0] * n[1] * n[2] > 2048 * 256) == (mesh_id != "7x9x11")
    mesh = box_mesh(n, dtype)()
    ctx = context_for(mesh)
    tdt = mesh.dtype.float
    g = torch.Generator().manual_seed(17)
    x_c = torch.randn(n, generator=g, dtype=torch.float64).to(tdt)
    y_c = torch.randn(n, generator=g, dtype=torch.float64).to(tdt)
    a = -0.7310585786300049

    def cpu(y, x):
        t = torch.tensor(a, dtype=tdt) * x      # the product, rounded in the mesh dtype ...
        return y + t                            # ... then the sum: two roundings

    x, y, out = x_c.cuda(), y_c.cuda(), torch.empty(n, dtype=tdt, device="cuda")
    assert torch.equal(ctx.vec_axpy(out, y, a, x).cpu(), cpu(y_c, x_c))          # no aliasing: the control
    y = y_c.cuda()
    assert ctx.vec_axpy(y, y, a, x) is y and torch.equal(y.cpu(), cpu(y_c, x_c)), "out is y"
    assert torch.equal(x.cpu(), x_c)
    y = y_c.cuda()
    assert torch.equal(ctx.vec_axpy(x, y, a, x).cpu(), cpu(y_c, x_c)), "out is x"
    assert torch.equal(y.cpu(), y_c)
    x = x_c.cuda()
    assert torch.equal(ctx.vec_axpy(x, x, a, x).cpu(), cpu(x_c, x_c)), "out is y is x"
