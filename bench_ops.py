#!/usr/bin/env python3
"""bench_ops.py -- secondary measurements for the other rows of SURVEY section 8 (not the driver's
contract; bench.py is).  One JSON line per workload: explicit Laplacian apply, the explicit
adv-diff Euler march (BASELINE config 4), the SSP Runge-Kutta march beside its unfused composition, the self-advected
march (div(phi, phi)) beside a frozen speed tensor and beside its step-by-step composition, the marches with a source term
(--sections source) beside the three-launch workaround and the generic kernel, the marches in a velocity field (--sections
velocity) beside the one-speed marches and the generic kernel, the momentum march of a vector field (--sections momentum)
beside three scalar marches in three frozen fields, the Euler step with a diffusivity field (--sections nu) beside the
constant-nu step and its torch composition, the two projection kernels (--sections projection) beside their compositions from
pa_grad, torch and apply_bcs, the pressure-carrying projection and the flow diagnostics (--sections pressure) beside the calls
and the torch passes they replace, Jacobi (config 1 and 3-D), BiCGSTAB, 2-D CG.
achieved GB/s uses the ALGORITHMIC bytes of SURVEY 8d (apply 2 passes, Euler 2-3, Jacobi 3,
CG 10, BiCGSTAB 22 = 2 applies x 2 + 9 axpy/dot passes x 2) against the 8 TB/s HBM peak.

    python bench_ops.py [--quick]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PEAK = 8000.0


def timed(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def emit(name, cells, ms, passes, esize, extra=None):
    gbs = passes * esize * cells / (ms * 1e-3) / 1e9
    out = {"workload": name, "ms": ms, "cell_updates_per_s": cells / (ms * 1e-3), "alg_passes": passes,
           "alg_GBs": gbs, "frac_of_hbm_peak": gbs / PEAK}
    if extra:
        out.update(extra)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--sections", default="ops,euler,rk,small,big",
                    help="comma-separated subset of: ops (explicit operators 512^3), euler (config 4 march), rk (SSP Runge-Kutta march, "
                         "fused stages against the composition of public pieces, then the self-advected march; self: those rows "
                         "alone; self_baselines: their two comparison rows alone, which need no self march in the library), "
                         "quick (the QUICK Euler step and order-3 march on k_sfq beside the generic kernel and beside upwind; not in "
                         "the default list; quick_baseline: the upwind rows alone, which a library without QUICK can run), tvd (rk_march orders 1 and 3 with "
                         "the slope-limited limiters minmod and mc, a scalar speed and a speed field, on k_sfq and with sfq 0, beside quick and "
                         "upwind, 256^3 fp32 config-4 BCs and 256^3 fp64 all-dirichlet; not in the default list; tvd_baseline: the quick and "
                         "upwind rows alone, which a library without the limiters can run), source (euler_march "
                         "and rk_march order 3 with a scalar source and a source field, beside no source, the euler_step + torch add + "
                         "apply_bcs workaround and the generic kernel; not in the default list; source_baseline: the no-source rows alone, "
                         "which a library without the source term can run), velocity (euler_march and rk_march order 3 with a "
                         "velocity of three equal scalars and of three fields, each on k_sf and with fastpath 0, beside the scalar-speed "
                         "and speed-tensor marches; not in the default list; velocity_baseline: the no-velocity rows alone, which a "
                         "library without the velocity entry points can run), momentum (momentum_march orders 1 and 3: the default, "
                         "vself 0, fastpath 0; not in the default list; momentum_baseline: the yardstick alone, three scalar rk_march "
                         "calls in three velocity fields, which a library without pa_momentum_march can run), nu (the Euler step with a diffusivity field at 256^3 and "
                         "512^3 fp32: tiled, generic, the constant-nu step and the torch composition; not in the default list), "
                         "projection (pa_divergence and pa_project_correct at 256^3 fp32 and fp64 beside their compositions from "
                         "pa_grad, torch and apply_bcs, and as a fraction of a device copy; not in the default list), "
                         "pressure (pa_project_update beside pa_project_correct + two pa_vec_axpy, pa_flow_stats beside its torch "
                         "composition, ns_step incremental beside chorin with the iteration counts, 256^3 fp32 and fp64; not in the "
                         "default list), "
                         "small (the reference's "
                         "own mesh sizes, resident vs launch per phase), big (Jacobi / BiCGSTAB 256^3, 2-D 4096^2, odd extents)")
    args = ap.parse_args()
    sections = set(args.sections.split(","))
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.fdc import FDC
    from pyapes_amd.solver.fdm import FDM
    from pyapes_amd.solver.march import euler_march, euler_step
    from pyapes_amd.solver.ops import Solver
    from pyapes_amd.testing.poisson import poisson_bcs, poisson_rhs_nd
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import homogeneous_bcs, mixed_bcs
    warnings.simplefilter("ignore")
    q = args.quick

    # --- explicit operators, 512^3: the C call on a pre-allocated output (no torch.empty, no Python wrapper
    #     beyond ctypes), fp64 and fp32.  Laplacian / Div: 2 passes; Grad: 1 read + 3 writes = 4 passes --------
    from pyapes_amd.hip import lib as L
    from pyapes_amd.hip.context import context_for
    n = 256 if q else 512
    for dt, es in ((("double", 8), ("single", 4)) if "ops" in sections else ()):
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", dt)
        var = Field("p", 1, mesh, {"domain": homogeneous_bcs(3, 0.0, "neumann"), "obstacle": None}, init_val="random")
        ctx = context_for(mesh)
        ctx.bind_bcs(var(), var.bcs, 0)
        x = var()[0]
        y = torch.empty_like(x)
        g3 = torch.empty((3, n, n, n), dtype=x.dtype, device=x.device)
        f = "f64" if dt == "double" else "f32"
        ms = timed(lambda: ctx.laplacian(x, False, out=y), 20)
        emit(f"laplacian apply {n}^3 {f} neumann (C call, pre-allocated output)", n ** 3, ms, 2, es)
        ms = timed(lambda: ctx.div(L.OP_DIV_UPWIND, 1.0, x, out=y), 20)
        emit(f"div apply {n}^3 {f} upwind, scalar speed (C call, pre-allocated output)", n ** 3, ms, 2, es)
        ms = timed(lambda: ctx.grad(x, False, out=g3), 20)
        emit(f"grad apply {n}^3 {f} -> 3 components (C call, pre-allocated output)", n ** 3, ms, 4, es)
        # the ceiling these are measured against: a device copy of the same array (1 read + 1 write)
        ms = timed(lambda: y.copy_(x), 20)
        emit(f"torch copy_ {n}^3 {f} (reference point: 1 read + 1 write)", n ** 3, ms, 2, es)
        del var, mesh, ctx, x, y, g3
        # every Div kind on the generic kernel (k_aop, "fastpath" 0) at 256^3, a scalar speed and a speed field; dirichlet
        # faces, which the central kind needs
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [256, 256, 256], "cuda", dt)
        var = Field("p", 1, mesh, {"domain": homogeneous_bcs(3, 0.0, "dirichlet"), "obstacle": None}, init_val="random")
        ctx = context_for(mesh)
        ctx.bind_bcs(var(), var.bcs, 0)
        ctx.set_option("fastpath", 0)
        x = var()[0]
        y, uf = torch.empty_like(x), torch.randn_like(x)
        for kname, kind in (("central", L.OP_DIV_CENTRAL), ("upwind compat", L.OP_DIV_UPWIND_COMPAT), ("upwind", L.OP_DIV_UPWIND),
                            ("quick", L.OP_DIV_QUICK), ("minmod", L.OP_DIV_MINMOD), ("mc", L.OP_DIV_MC)):
            for uname, u, passes in (("scalar speed", 0.7, 2), ("speed field", uf, 3)):
                ms = timed(lambda: ctx.div(kind, u, x, out=y), 20)
                emit(f"div apply 256^3 {f} {kname}, {uname}, fastpath 0 (k_aop)", 256 ** 3, ms, passes, es)
        ctx.set_option("fastpath", 1)
        del var, mesh, ctx, x, y, uf

    # --- config 4: explicit adv-diff march 256^3 fp32, upwind, Neumann / Symmetry ------------------
    if "euler" in sections:
        euler_rows(q, emit)
    if "rk" in sections:
        rk_rows(q, emit)
    if sections & {"quick", "quick_baseline"}:
        quick_rows(q, emit, with_quick="quick" in sections)
    if sections & {"tvd", "tvd_baseline"}:
        tvd_rows(q, emit, with_tvd="tvd" in sections)
    if sections & {"rk", "self", "self_baselines"}:
        self_rows(q, emit, with_self=bool(sections & {"rk", "self"}))
    if sections & {"source", "source_baseline"}:
        source_rows(q, emit, with_source="source" in sections)
    if sections & {"velocity", "velocity_baseline"}:
        velocity_rows(q, emit, with_velocity="velocity" in sections)
    if sections & {"momentum", "momentum_baseline"}:
        momentum_rows(q, emit, with_momentum="momentum" in sections)
    if "nu" in sections:
        nu_rows(q, emit)
    if "projection" in sections:
        projection_rows(q, emit)
    if "pressure" in sections:
        pressure_rows(q, emit)
    solver_rows(q, emit, sections)


def projection_rows(q, emit):
    """The two streaming kernels of the pressure projection at 256^3, fp32 and fp64, all-dirichlet faces, on pre-allocated
    outputs: ``pa_divergence`` (d + 1 = 4 arrays) beside its composition from existing entry points -- ``pa_grad`` of every
    component into a (3, 3, *n) buffer, the diagonal summed and scaled in torch -- and ``pa_project_correct`` with its BC fills
    (2 d + 1 = 7 arrays) beside ``pa_grad(p)``, three torch updates of U and ``apply_bcs``.  Every variant is timed three times
    in alternation; ms is the median, ms_all the three.  ``frac_of_copy``: the algorithmic bytes per second over those of a
    device copy of one array of the mesh (1 read + 1 write), measured in the same alternation."""
    from pyapes_amd.geometry import Box
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    n = 128 if q else 256
    for dt, es in (("single", 4), ("double", 8)):
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", dt)
        vals = [[0.0, 0.0, 0.0]] * 5 + [[1.0, 0.5, 0.0]]
        Uf = Field("U", 3, mesh, {"domain": mixed_bcs(vals, ["dirichlet"] * 6), "obstacle": None}, init_val="random")
        Uf.apply_bcs()
        ctx = context_for(mesh)
        U = Uf()
        g = torch.Generator(device="cuda").manual_seed(0)
        p = torch.rand((n, n, n), generator=g, device="cuda", dtype=U.dtype)
        d, d2 = torch.empty_like(p), torch.empty_like(p)
        g9 = torch.empty((3, 3, n, n, n), dtype=U.dtype, device="cuda")
        g3 = g9[0]
        scale, cscale = 1.0 / 0.01, 1e-6
        ctx.bind_bcs(U, Uf.bcs, 0)

        def fused_div():
            ctx.divergence(U, scale, out=d)

        def composed_div():
            for c in range(3):
                ctx.grad(U[c], False, out=g9[c])
            torch.add(g9[0][0], g9[1][1], out=d2)
            d2.add_(g9[2][2])
            d2.mul_(scale)

        def fused_correct():
            ctx.project_correct(U, p, cscale, Uf.bcs)

        def composed_correct():
            ctx.grad(p, False, out=g3)
            for c in range(3):
                U[c].sub_(g3[c], alpha=cscale)
            Uf.apply_bcs()

        def copy():
            d.copy_(p)

        rows = [("divergence, fused k_divergence", fused_div, 4, 100),
                ("divergence, composed: pa_grad per component + torch sums", composed_div, 4, 20),
                ("project_correct, fused k_project_correct + BC fills", fused_correct, 7, 100),
                ("project_correct, composed: pa_grad(p) + torch updates + apply_bcs", composed_correct, 7, 20),
                ("torch copy_ of one array (reference point: 1 read + 1 write)", copy, 2, 100)]
        ms = {name: [] for name, *_ in rows}
        for _ in range(3):
            for name, fn, _, iters in rows:
                ms[name].append(timed(fn, iters))
        med = {name: sorted(v)[1] for name, v in ms.items()}
        copy_gbs = 2 * es * n ** 3 / (med[rows[4][0]] * 1e-3) / 1e9
        f = "f64" if dt == "double" else "f32"
        for k, (name, _, passes, _) in enumerate(rows):
            extra = {"ms_all": ms[name], "frac_of_copy": passes * es * n ** 3 / (med[name] * 1e-3) / 1e9 / copy_gbs}
            if k in (0, 2):
                extra["speedup_over_composition"] = med[rows[k + 1][0]] / med[name]
            emit(f"{name} {n}^3 {f}, dirichlet", n ** 3, med[name], passes, es, extra)
        assert bool(torch.isfinite(U).all()) and bool(torch.isfinite(d).all())
        del Uf, mesh, ctx, U, p, d, d2, g9, g3


def pressure_rows(q, emit):
    """The pressure-carrying projection at 256^3, fp32 and fp64, on pre-allocated buffers.  ``pa_project_update`` in its
    rotational form with the BC fills of U (2 d + 4 = 10 arrays, one launch) beside the sequence it replaces,
    ``pa_project_correct`` with those fills and two ``pa_vec_axpy`` (2 d + 7 = 13 arrays, three launches).  ``pa_flow_stats``
    (d = 3 arrays read, one synchronise) beside the torch composition of the same four numbers with one synchronise (rolls,
    elementwise passes and reductions; counted as 3 arrays too: the bytes that have to move).  Then ``ns_step`` on one flow --
    a lid-driven box with an outflow face, from p = 0 -- four steps per run, "incremental" beside "chorin", CG to 1e-6 with at
    most 4000 iterations: ms per step and the iteration counts of every step.  Every variant is timed three times in alternation; ms is the median,
    ms_all the three."""
    import math

    from pyapes_amd.geometry import Box
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.projection import ns_step
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    n = 128 if q else 256
    for dt, es in (("single", 4), ("double", 8)):
        f = "f64" if dt == "double" else "f32"
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", dt)
        uvals = [[0.0, 0.0, 0.0]] * 5 + [[1.0, 0.5, 0.0]]
        utypes = ["dirichlet", "neumann"] + ["dirichlet"] * 4
        ubc = {"domain": mixed_bcs(uvals, utypes), "obstacle": None}
        pbc = {"domain": mixed_bcs([0.0] * 6, ["neumann", "dirichlet"] + ["neumann"] * 4), "obstacle": None}
        Uf = Field("U", 3, mesh, ubc, init_val="random")
        Uf.apply_bcs()
        ctx = context_for(mesh)
        U = Uf()
        g = torch.Generator(device="cuda").manual_seed(0)
        p, phi, r = (torch.rand((n, n, n), generator=g, device="cuda", dtype=U.dtype) for _ in range(3))
        U2, p2 = U.clone(), p.clone()
        cscale, chi = 1e-6, 1e-7
        ctx.bind_bcs(U, Uf.bcs, 0)
        ih = [1.0 / float(h) for h in mesh.dx_list]

        def fused_update():
            ctx.project_update(U, phi, cscale, p, r, chi, Uf.bcs)

        def composed_update():
            ctx.project_correct(U2, phi, cscale, Uf.bcs)
            ctx.vec_axpy(p2, p2, 1.0, phi)
            ctx.vec_axpy(p2, p2, chi, r)

        def fused_stats():
            ctx.flow_stats(U)

        def torch_stats():
            rate = U[0].abs() * ih[0] + U[1].abs() * ih[1] + U[2].abs() * ih[2]
            div = sum((torch.roll(U[a], -1, a) - torch.roll(U[a], 1, a)) * (0.5 * ih[a]) for a in range(3))[1:-1, 1:-1, 1:-1]
            torch.stack([rate.max().double(), div.abs().max().double(), (div * div).sum(dtype=torch.float64),
                         (U * U).sum(dtype=torch.float64)]).tolist()

        rows = [("project_update (rotational), fused k_project_update + BC fills", fused_update, 10, 400),
                ("project_update, composed: pa_project_correct + BC fills + two pa_vec_axpy", composed_update, 13, 400),
                ("flow_stats, fused k_flow_stats", fused_stats, 3, 400),
                ("flow_stats, composed: torch rolls, elementwise passes and reductions", torch_stats, 3, 40)]
        ms = {name: [] for name, *_ in rows}
        for _ in range(3):
            for name, fn, _, iters in rows:
                ms[name].append(timed(fn, iters))
        med = {name: sorted(v)[1] for name, v in ms.items()}
        for k, (name, _, passes, _) in enumerate(rows):
            extra = {"ms_all": ms[name]}
            if k in (0, 2):
                extra["speedup_over_composition"] = med[rows[k + 1][0]] / med[name]
            emit(f"{name} {n}^3 {f}", n ** 3, med[name], passes, es, extra)
        assert bool(torch.isfinite(U).all()) and bool(torch.isfinite(p).all())
        del U2, p2, phi, r

        # ns_step on one flow: the lid sets a box of fluid at rest in motion
        X, Y, Z = mesh.X, mesh.Y, mesh.Z
        U0 = torch.stack([torch.sin(math.pi * X) * torch.cos(math.pi * Y) * Z, -torch.cos(math.pi * X) * torch.sin(math.pi * Y) * Z,
                          0.1 * torch.sin(math.pi * Z) * X]).to(U.dtype).contiguous()
        nu, step, nsteps = 1e-3, 0.2 * float(mesh.dx_list[0]), 4
        solver = {"fdm": {"method": "cg", "tol": 1e-6, "max_it": 4000, "report": False}}

        def run(form):
            Ug, pg = Field("U", 3, mesh, ubc), Field("p", 1, mesh, pbc)
            Ug.set_var_tensor(U0.clone())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            itr = [ns_step(Ug, pg, nu, step, None, 3, rho=1.0, solver=solver, form=form)["itr"] for _ in range(nsteps)]
            torch.cuda.synchronize()
            assert bool(torch.isfinite(Ug()).all())
            return (time.perf_counter() - t0) * 1e3 / nsteps, itr

        run("incremental")                                   # warm: work tensors, the solver's scratch
        res = {"chorin": [], "incremental": []}
        for _ in range(3):
            for form in res:
                res[form].append(run(form))
        meds = {form: sorted(v)[1][0] for form, v in res.items()}
        for form, v in res.items():
            extra = {"ms_all": [m for m, _ in v], "itr_per_step": v[0][1], "steps": nsteps}
            if form == "incremental":
                extra["speedup_over_chorin"] = meds["chorin"] / meds[form]
            emit(f"ns_step {form}, lid-driven box, order 3, CG tol 1e-6 max_it 4000, per step {n}^3 {f}", n ** 3, meds[form], 0, es, extra)
        del Uf, mesh, ctx, U, p, U0


def nu_rows(q, emit):
    """The Euler step with a diffusivity FIELD, div(nu grad phi) - upwind div(u phi), u = 0.7, all-dirichlet faces, fp32, on a
    pre-allocated output (step kernel + BC fill per call): the tiled k_sfn, the generic k_euler (option sf 0), the constant-nu step
    on k_sf on the same mesh (one array fewer: a floor) and the torch composition of the same term -- rolls and elementwise
    operations plus apply_bcs, what a caller has to write without the feature.  Every variant is timed three times in
    alternation; ms is the median, ms_all the three."""
    from pyapes_amd.geometry import Box
    from pyapes_amd.hip import lib as L
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import homogeneous_bcs
    for n in ((128,) if q else (256, 512)):
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", "single")
        phi = Field("phi", 1, mesh, {"domain": homogeneous_bcs(3, 0.0, "dirichlet"), "obstacle": None})
        phi.set_var_tensor(torch.exp(-((mesh.X - 0.5) ** 2 + (mesh.Y - 0.5) ** 2 + (mesh.Z - 0.5) ** 2) / 0.02)
                           .unsqueeze(0).contiguous())
        phi.apply_bcs()
        ctx = context_for(mesh)
        ctx.bind_bcs(phi(), phi.bcs, 0)
        g = torch.Generator(device="cuda").manual_seed(0)
        nu = (1e-3 * (0.5 + torch.rand((n, n, n), generator=g, device="cuda", dtype=torch.float32))).contiguous()
        dx = float(mesh.dx_list[0])
        dt, u = 0.2 * min(dx * dx / (6 * 1.5e-3), dx / 1.0), 0.7
        x, out = phi()[0], torch.empty_like(phi()[0])
        w, ih = 0.5 / (dx * dx), 1.0 / dx
        scratch = Field("t", 1, mesh, {"domain": homogeneous_bcs(3, 0.0, "dirichlet"), "obstacle": None})

        def torch_step():
            d = torch.zeros_like(x)
            adv = torch.zeros_like(x)
            for a in range(3):
                fp = torch.roll(x, -1, a) - x
                fm = x - torch.roll(x, 1, a)
                d = d + ((torch.roll(nu, -1, a) + nu) * fp - (nu + torch.roll(nu, 1, a)) * fm) * w
                adv = adv + (u * fm) * ih
            scratch.set_var_tensor((x + dt * (d - adv)).unsqueeze(0))
            scratch.apply_bcs()

        def tiled():
            ctx.step_nu(x, None, out, 0.0, 0.0, L.OP_DIV_UPWIND, u, nu, dt)

        def generic():
            ctx.set_option("sf", 0)
            ctx.step_nu(x, None, out, 0.0, 0.0, L.OP_DIV_UPWIND, u, nu, dt)
            ctx.set_option("sf", 1)

        def constant():
            ctx.euler_step(x, out, L.OP_DIV_UPWIND, u, 1e-3, dt)

        rows = [("nu-field step, tiled k_sfn", tiled, 3, 100), ("nu-field step, generic k_euler (sf 0)", generic, 3, 100),
                ("constant-nu step, k_sf (yardstick: one array fewer)", constant, 2, 100),
                ("torch composition of the nu-field step (rolls + elementwise + apply_bcs)", torch_step, 3, 10)]
        ms = {name: [] for name, *_ in rows}
        for _ in range(3):
            for name, fn, _, iters in rows:
                ms[name].append(timed(fn, iters if n <= 256 else max(iters // 4, 5)))
        for name, _, passes, _ in rows:
            emit(f"{name} {n}^3 f32 upwind u 0.7, dirichlet", n ** 3, sorted(ms[name])[1], passes, 4, {"ms_all": ms[name]})
        assert bool(torch.isfinite(out).all())
        del phi, scratch, mesh, ctx, nu, x, out


def euler_rows(q, emit):
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.march import euler_march, euler_step
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    n = 128 if q else 256
    mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", "single")
    bcs = mixed_bcs([0.0, 0.0, None, None, None, None],
                    ["neumann", "neumann", "symmetry", "symmetry", "symmetry", "symmetry"])
    phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
    phi.set_var_tensor(torch.exp(-((mesh.X - 0.5) ** 2 + (mesh.Y - 0.5) ** 2 + (mesh.Z - 0.5) ** 2) / 0.02)
                       .unsqueeze(0).contiguous())
    phi.apply_bcs()
    nu = 1e-3
    dx = mesh.dx_list[0]
    dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.0)
    cfg = {"div": {"limiter": "upwind"}}
    ms = timed(lambda: euler_step(phi, 1.0, nu, dt, cfg), 100)
    emit(f"euler adv-diff step {n}^3 f32 upwind scalar u, neumann/symmetry (config 4)", n ** 3, ms, 2, 4)
    ut = torch.ones_like(phi()) * 0.7
    ms = timed(lambda: euler_step(phi, ut, nu, dt, cfg), 100)
    emit(f"euler adv-diff step {n}^3 f32 upwind speed tensor (config 4)", n ** 3, ms, 3, 4)
    ms = timed(lambda: euler_march(phi, 1.0, nu, dt, 50, cfg), 4) / 50
    emit(f"euler_march (50 steps per call) {n}^3 f32 upwind scalar u (config 4)", n ** 3, ms, 2, 4)
    ms = timed(lambda: euler_march(phi, ut, nu, dt, 50, cfg), 4) / 50
    emit(f"euler_march (50 steps per call) {n}^3 f32 upwind speed tensor (config 4)", n ** 3, ms, 3, 4)
    assert bool(torch.isfinite(phi()).all())
    del phi, mesh, ut
    if not q:   # the same march at 512^3 fp32: 512 MiB per array, outside the 256 MiB Infinity Cache
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [512, 512, 512], "cuda", "single")
        phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
        phi.set_var_tensor(torch.exp(-((mesh.X - 0.5) ** 2 + (mesh.Y - 0.5) ** 2 + (mesh.Z - 0.5) ** 2) / 0.02)
                           .unsqueeze(0).contiguous())
        phi.apply_bcs()
        dx = mesh.dx_list[0]
        dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.0)
        ms = timed(lambda: euler_march(phi, 1.0, nu, dt, 20, cfg), 3) / 20
        emit("euler_march (20 steps per call) 512^3 f32 upwind scalar u", 512 ** 3, ms, 2, 4)
        del phi, mesh

def rk_rows(q, emit):
    """rk_march (one C call per march: Euler kernel + one fused stage kernel per further stage) beside the same march made
    of public pieces that need no stage kernel: euler_step, c0 * phi0 + c1 * E as torch ops, apply_bcs.  ms per STEP.
    Algorithmic passes of a step: its Euler stage 2, every fused stage 3 (phi_s, phi0 in, one out), + 1 each with a
    speed tensor -- order 3: 8 (11), order 2: 5 (7)."""
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.march import SSP_STAGES, euler_step, rk_march
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    bcs = mixed_bcs([0.0, 0.0, None, None, None, None],
                    ["neumann", "neumann", "symmetry", "symmetry", "symmetry", "symmetry"])
    cfg = {"div": {"limiter": "upwind"}}
    nu, steps = 1e-3, 20

    def unfused_march(phi, u, dt, order):
        for _ in range(steps):
            phi0 = phi()            # euler_step hands phi a new tensor: this one stays what it is
            euler_step(phi, u, nu, dt, cfg)
            for c0, c1 in SSP_STAGES[order]:
                euler_step(phi, u, nu, dt, cfg)
                phi.set_var_tensor(c0 * phi0 + c1 * phi())
                phi.apply_bcs()

    sizes = [(128, "single")] if q else [(256, "single"), (512, "single"), (256, "double")]
    for n, dtype in sizes:
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", dtype)
        es, f = (8, "f64") if dtype == "double" else (4, "f32")
        start = torch.exp(-((mesh.X - 0.5) ** 2 + (mesh.Y - 0.5) ** 2 + (mesh.Z - 0.5) ** 2) / 0.02).unsqueeze(0).contiguous()
        dx = mesh.dx_list[0]
        dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.0)
        ut = torch.ones_like(start) * 0.7
        for order in (3, 2):
            for uname, u, extra in (("scalar u", 1.0, 0), ("speed tensor", ut, 1)):
                phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
                phi.set_var_tensor(start.clone())
                phi.apply_bcs()
                passes = 2 + 3 * (order - 1) + extra * order
                ms_f = timed(lambda: rk_march(phi, u, nu, dt, steps, cfg, order=order), 3, warm=1) / steps
                emit(f"rk_march order {order} ({steps} steps per call) {n}^3 {f} upwind {uname} (config 4 BCs)", n ** 3, ms_f, passes, es)
                ms_u = timed(lambda: unfused_march(phi, u, dt, order), 3, warm=1) / steps
                emit(f"unfused order {order} (euler_step + torch combine + apply_bcs, {steps} steps) {n}^3 {f} upwind {uname}", n ** 3,
                     ms_u, passes, es, {"fused_over_unfused": ms_f / ms_u})
                assert bool(torch.isfinite(phi()).all())
                del phi
        del mesh, start, ut
        torch.cuda.empty_cache()


def quick_rows(q, emit, with_quick=True):
    """Div limiter "quick" (k_sfq, csrc/pa_sfq_kernel.h) with the config-4 BCs, fp32: the Euler step with a scalar speed and with a
    speed tensor, and rk_march order 3 (20 steps per call, ms per STEP) -- each beside (a) the upwind row with "bcl": 0 (step +
    fill per launch, what QUICK does too) and (b) QUICK on the generic kernel ("sfq": 0); "sfq": 2 / 4 force the rows per
    wave.  The variants of a row are timed in turn, three rounds; "ms" is the median, "ms_rounds" all three.  Algorithmic
    passes as for upwind: step 2 (3 with a speed tensor), order-3 step 8."""
    from pyapes_amd.geometry import Box
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.march import euler_step, rk_march
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    bcs = mixed_bcs([0.0, 0.0, None, None, None, None],
                    ["neumann", "neumann", "symmetry", "symmetry", "symmetry", "symmetry"])
    up, qk = {"div": {"limiter": "upwind"}}, {"div": {"limiter": "quick"}}
    nu, steps = 1e-3, 20
    variants = [("upwind bcl 0", up, {"bcl": 0, "sfq": 1}), ("quick", qk, {"bcl": 1, "sfq": 1}), ("quick sfq 0", qk, {"sfq": 0}),
                ("quick sfq 2", qk, {"sfq": 2}), ("quick sfq 4", qk, {"sfq": 4})]
    if not with_quick:   # (a library from before QUICK knows neither the kind nor the option)
        variants = [("upwind bcl 0", up, {"bcl": 0})]
    for n in ([128] if q else [256, 512]):
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", "single")
        ctx = context_for(mesh)
        start = torch.exp(-((mesh.X - 0.5) ** 2 + (mesh.Y - 0.5) ** 2 + (mesh.Z - 0.5) ** 2) / 0.02).unsqueeze(0).contiguous()
        dx = mesh.dx_list[0]
        dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.0)
        ut = torch.ones_like(start) * 0.7
        iters = 400 if n <= 256 else 60
        works = [("euler step", "scalar u", 2, lambda phi, cfg: timed(lambda: euler_step(phi, 1.0, nu, dt, cfg), iters, warm=5)),
                 ("euler step", "speed tensor", 3, lambda phi, cfg: timed(lambda: euler_step(phi, ut, nu, dt, cfg), iters, warm=5)),
                 (f"rk_march order 3 ({steps} steps per call)", "scalar u", 8,
                  lambda phi, cfg: timed(lambda: rk_march(phi, 1.0, nu, dt, steps, cfg, order=3), 3 if n <= 256 else 1, warm=1) / steps)]
        for what, uname, passes, run in works:
            rounds = {v[0]: [] for v in variants}
            for _ in range(3):
                for vname, cfg, opts in variants:
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
                    phi.set_var_tensor(start.clone())
                    phi.apply_bcs()
                    rounds[vname].append(run(phi, cfg))
                    assert bool(torch.isfinite(phi()).all())
                    del phi
            base = sorted(rounds["upwind bcl 0"])[1]
            for vname, _, opts in variants:
                ms = sorted(rounds[vname])[1]
                emit(f"{what} {n}^3 f32 {vname} {uname} (config 4 BCs)", n ** 3, ms, passes, 4,
                     {"ms_rounds": rounds[vname], "over_upwind_bcl0": ms / base, "options": opts})
        for k, v in (("sfq", 1), ("bcl", 1)) if with_quick else (("bcl", 1),):
            ctx.set_option(k, v)
        del mesh, start, ut
        torch.cuda.empty_cache()


def tvd_rows(q, emit, with_tvd=True):
    """Div limiters "minmod" and "mc" (the SCH instantiations of k_sfq, csrc/pa_sft.hip): rk_march of orders 1 and 3 with a scalar
    speed and with a speed field, 256^3 fp32 with the config-4 BCs and 256^3 fp64 all-dirichlet -- each limiter on k_sfq and on the
    generic kernel ("sfq": 0), beside "quick" (same footprint, same streams), "quick" with "sfq": 0 and "upwind" with "bcl": 0 (step
    + fill per launch, what the schemes with a reach of 2 do too).  One sample is ONE march of 20 steps (ms per STEP); the variants
    of a row are timed in turn, five rounds after a warm-up march each: "ms" is the median, "ms_min" the minimum, "ms_rounds" all
    five.  Algorithmic passes as for upwind: per Euler stage 2 (3 with a speed field), the two fused stages of order 3 read phi0
    as well."""
    from pyapes_amd.geometry import Box
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.march import rk_march
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    cfg = {lim: {"div": {"limiter": lim}} for lim in ("upwind", "quick", "minmod", "mc")}
    nu, steps, rounds_n = 1e-3, 20, 5
    variants = [("upwind bcl 0", "upwind", {"bcl": 0, "sfq": 1}), ("quick", "quick", {"bcl": 1, "sfq": 1}), ("quick sfq 0", "quick", {"sfq": 0})]
    if with_tvd:   # (a library from before the limiters does not know the kinds)
        variants += [("minmod", "minmod", {"sfq": 1}), ("minmod sfq 0", "minmod", {"sfq": 0}), ("mc", "mc", {"sfq": 1}),
                     ("mc sfq 0", "mc", {"sfq": 0})]
    n = 128 if q else 256
    setups = [("single", "f32", 4, "config 4 BCs", mixed_bcs([0.0, 0.0, None, None, None, None],
                                                           ["neumann", "neumann", "symmetry", "symmetry", "symmetry", "symmetry"])),
              ("double", "f64", 8, "all dirichlet", mixed_bcs([0.0] * 6, ["dirichlet"] * 6))]
    for dtype, fname, esize, bcname, bcs in setups:
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", dtype)
        ctx = context_for(mesh)
        start = torch.exp(-((mesh.X - 0.5) ** 2 + (mesh.Y - 0.5) ** 2 + (mesh.Z - 0.5) ** 2) / 0.02).unsqueeze(0).contiguous()
        dx = mesh.dx_list[0]
        dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.0)
        ut = (0.7 * torch.cos(6.0 * mesh.X) * torch.cos(4.0 * mesh.Y + 2.0 * mesh.Z)).unsqueeze(0).contiguous()   # both signs
        for order in (1, 3):
            for uname, u, passes in (("scalar u", 1.0, 2 if order == 1 else 8), ("speed field", ut, 3 if order == 1 else 11)):
                def one_march(lim):
                    phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
                    phi.set_var_tensor(start.clone())
                    phi.apply_bcs()
                    ms = timed(lambda: rk_march(phi, u, nu, dt, steps, cfg[lim], order=order), 1, warm=0) / steps
                    assert bool(torch.isfinite(phi()).all())
                    return ms
                rounds = {v[0]: [] for v in variants}
                for r in range(rounds_n + 1):        # round 0: the warm-up march of every variant
                    for vname, lim, opts in variants:
                        for k, v in opts.items():
                            ctx.set_option(k, v)
                        ms = one_march(lim)
                        if r:
                            rounds[vname].append(ms)
                base = sorted(rounds["quick"])[rounds_n // 2]
                for vname, lim, opts in variants:
                    ms = sorted(rounds[vname])[rounds_n // 2]
                    emit(f"rk_march order {order} ({steps} steps per call) {n}^3 {fname} {vname} {uname} ({bcname})", n ** 3, ms, passes,
                         esize, {"ms_min": min(rounds[vname]), "ms_rounds": rounds[vname], "over_quick": ms / base, "options": opts})
        for k, v in (("sfq", 1), ("bcl", 1)):
            ctx.set_option(k, v)
        del mesh, start, ut
        torch.cuda.empty_cache()


def source_rows(q, emit, with_source=True):
    """The source term S of the marches (``source=``; the SRC instantiations of k_sf, csrc/pa_sf_kernel.h), upwind, config-4
    BCs, fp32: euler_march and rk_march order 3 (20 steps per call, ms per STEP) without a source, with a scalar source, with
    a source field, with a source field on the generic kernel ("fastpath": 0) and -- the Euler rows -- beside what a user
    could do before: euler_step, a torch add of dt * S on the interior set, apply_bcs, per step.  The variants of a row are
    timed in turn, three rounds; "ms" is the median, "ms_rounds" all three.  Algorithmic passes: Euler step 2, order-3 step
    8, + 1 per launch with a source field."""
    from pyapes_amd.geometry import Box
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.march import euler_march, euler_step, rk_march
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    bcs = mixed_bcs([0.0, 0.0, None, None, None, None],
                    ["neumann", "neumann", "symmetry", "symmetry", "symmetry", "symmetry"])
    cfg = {"div": {"limiter": "upwind"}}
    nu, steps = 1e-3, 20
    for n in ([128] if q else [256, 512]):
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", "single")
        ctx = context_for(mesh)
        start = torch.exp(-((mesh.X - 0.5) ** 2 + (mesh.Y - 0.5) ** 2 + (mesh.Z - 0.5) ** 2) / 0.02).unsqueeze(0).contiguous()
        dx = mesh.dx_list[0]
        dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.0)
        S = (torch.sin(3.0 * mesh.X) * torch.cos(2.0 * mesh.Y)).unsqueeze(0).contiguous()
        dtS = (dt * S)[0][1:-1, 1:-1, 1:-1].contiguous()
        reps = 3 if n <= 256 else 1

        def workaround(phi):
            for _ in range(steps):
                euler_step(phi, 1.0, nu, dt, cfg)
                phi()[0][1:-1, 1:-1, 1:-1] += dtS
                phi.apply_bcs()

        def euler(src):
            return lambda phi: timed(lambda: euler_march(phi, 1.0, nu, dt, steps, cfg, **src), reps, warm=1) / steps

        def rk3(src):
            return lambda phi: timed(lambda: rk_march(phi, 1.0, nu, dt, steps, cfg, order=3, **src), reps, warm=1) / steps

        for what, make, lanes, base_passes in ((f"euler_march ({steps} steps per call)", euler, 1, 2),
                                               (f"rk_march order 3 ({steps} steps per call)", rk3, 3, 8)):
            variants = [("no source", make({}), {"fastpath": 1}, base_passes)]
            if with_source:   # (a library from before the source term has no entry point that takes one)
                variants += [("scalar source", make({"source": 0.5}), {"fastpath": 1}, base_passes),
                             ("source field", make({"source": S}), {"fastpath": 1}, base_passes + lanes),
                             ("source field fastpath 0", make({"source": S}), {"fastpath": 0}, base_passes + lanes)]
                if lanes == 1:
                    variants.append(("workaround euler_step + torch interior add + apply_bcs",
                                     lambda phi: timed(lambda: workaround(phi), reps, warm=1) / steps, {"fastpath": 1}, 5))
            rounds = {v[0]: [] for v in variants}
            for _ in range(3):
                for vname, run, opts, _ in variants:
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
                    phi.set_var_tensor(start.clone())
                    phi.apply_bcs()
                    rounds[vname].append(run(phi))
                    assert bool(torch.isfinite(phi()).all())
                    del phi
            base = sorted(rounds["no source"])[1]
            for vname, _, opts, passes in variants:
                ms = sorted(rounds[vname])[1]
                emit(f"{what} {n}^3 f32 upwind scalar u, {vname} (config 4 BCs)", n ** 3, ms, passes, 4,
                     {"ms_rounds": rounds[vname], "over_no_source": ms / base, "options": opts})
        ctx.set_option("fastpath", 1)
        del mesh, start, S, dtS
        torch.cuda.empty_cache()


def velocity_rows(q, emit, with_velocity=True):
    """The marches in a velocity field, one advection speed per mesh axis (``u`` a tuple; the VEL instantiations of k_sf,
    csrc/pa_sf_kernel.h), upwind, config-4 BCs, fp32: euler_march and rk_march order 3 (20 steps per call, ms per STEP).  The
    no-velocity rows: a scalar speed with "bcl": 0 (a velocity march fills per step or stage, so that is its like-for-like
    twin), and a speed tensor with and without BC on load.  The velocity rows: three equal scalars (beside the scalar-speed
    row) and three fields (beside the speed-tensor row), each on k_sf and on the generic kernel ("fastpath": 0).  The
    variants of a row are timed in turn, three rounds; "ms" is the median, "ms_rounds" all three.  Algorithmic passes per
    launch: 2, + 1 for a speed tensor, + 3 for three velocity fields, + 1 for phi0 in a stage (12 -> 20 B per cell in fp32
    for the Euler step with a speed tensor -> three fields)."""
    from pyapes_amd.geometry import Box
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.march import euler_march, rk_march
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    bcs = mixed_bcs([0.0, 0.0, None, None, None, None],
                    ["neumann", "neumann", "symmetry", "symmetry", "symmetry", "symmetry"])
    cfg = {"div": {"limiter": "upwind"}}
    nu, steps = 1e-3, 20
    for n in ([128] if q else [256, 512]):
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", "single")
        ctx = context_for(mesh)
        start = torch.exp(-((mesh.X - 0.5) ** 2 + (mesh.Y - 0.5) ** 2 + (mesh.Z - 0.5) ** 2) / 0.02).unsqueeze(0).contiguous()
        dx = mesh.dx_list[0]
        dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.0)
        U = (0.5 + 0.5 * torch.sin(3.0 * mesh.X) * torch.cos(2.0 * mesh.Y)).unsqueeze(0).contiguous()   # 0 <= u <= 1
        V3 = (U[0], (0.8 * torch.cos(2.0 * mesh.Z)).contiguous(), (-0.6 * torch.sin(mesh.X + mesh.Y)).contiguous())
        reps = 3 if n <= 256 else 1

        def euler(u):
            return lambda phi: timed(lambda: euler_march(phi, u, nu, dt, steps, cfg), reps, warm=1) / steps

        def rk3(u):
            return lambda phi: timed(lambda: rk_march(phi, u, nu, dt, steps, cfg, order=3), reps, warm=1) / steps

        for what, make, launches, extra0 in ((f"euler_march ({steps} steps per call)", euler, 1, 0),
                                             (f"rk_march order 3 ({steps} steps per call)", rk3, 3, 2)):
            base_passes = 2 * launches + extra0
            variants = [("scalar speed, bcl 0", make(1.0), {"fastpath": 1, "bcl": 0}, base_passes),
                        ("speed tensor", make(U), {"fastpath": 1, "bcl": 1}, base_passes + launches),
                        ("speed tensor, bcl 0", make(U), {"fastpath": 1, "bcl": 0}, base_passes + launches)]
            if with_velocity:   # (a library from before the velocity has no entry point that takes one)
                variants += [("velocity of three equal scalars", make((1.0, 1.0, 1.0)), {"fastpath": 1, "bcl": 1}, base_passes),
                             ("velocity of three equal scalars, fastpath 0", make((1.0, 1.0, 1.0)), {"fastpath": 0, "bcl": 1}, base_passes),
                             ("velocity of three fields", make(V3), {"fastpath": 1, "bcl": 1}, base_passes + 3 * launches),
                             ("velocity of three fields, fastpath 0", make(V3), {"fastpath": 0, "bcl": 1}, base_passes + 3 * launches)]
            rounds = {v[0]: [] for v in variants}
            for _ in range(3):
                for vname, run, opts, _ in variants:
                    for k, v in opts.items():
                        ctx.set_option(k, v)
                    phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
                    phi.set_var_tensor(start.clone())
                    phi.apply_bcs()
                    rounds[vname].append(run(phi))
                    assert bool(torch.isfinite(phi()).all())
                    del phi
            scalar = sorted(rounds["scalar speed, bcl 0"])[1]
            tensor = sorted(rounds["speed tensor, bcl 0"])[1]
            for vname, _, opts, passes in variants:
                ms = sorted(rounds[vname])[1]
                emit(f"{what} {n}^3 f32 upwind, {vname} (config 4 BCs)", n ** 3, ms, passes, 4,
                     {"ms_rounds": rounds[vname], "over_scalar_speed_bcl0": ms / scalar, "over_speed_tensor_bcl0": ms / tensor,
                      "options": opts})
        ctx.set_option("fastpath", 1)
        ctx.set_option("bcl", 1)
        del mesh, start, U, V3
        torch.cuda.empty_cache()


def momentum_rows(q, emit, with_momentum=True):
    """``momentum_march`` -- a vector field that advects itself, one launch per stage and component (pa_momentum_march) --
    upwind, config-4 BC types, fp32, orders 1 and 3 (20 steps per call, ms per STEP): the default (k_sf VEL 3), "vself": 0
    (the aliased VEL 2 instantiations) and "fastpath": 0 (the generic kernel).  The yardstick: three scalar ``rk_march`` calls,
    one per component, in three FROZEN velocity fields (VEL 2) -- what a user could run before, and all a library without
    pa_momentum_march can run (momentum_baseline).  Variants are timed in turn, three rounds; "ms" is the median.  Passes per
    launch: 2 + 2 speed fields (VEL 3; 3 for VEL 2 and the generic kernel, which re-read the target as a speed), + 1 for phi0
    in a stage."""
    from pyapes_amd.geometry import Box
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.march import rk_march
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    types = ["neumann", "neumann", "symmetry", "symmetry", "symmetry", "symmetry"]
    bcs = mixed_bcs([0.0, 0.0, None, None, None, None], types)
    vbcs = mixed_bcs([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], None, None, None, None], types)
    cfg = {"div": {"limiter": "upwind"}}
    nu, steps = 1e-3, 20
    for n in ([128] if q else [256, 512]):
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", "single")
        ctx = context_for(mesh)
        dx = mesh.dx_list[0]
        dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.0)
        V3 = torch.stack([0.5 + 0.5 * torch.sin(3.0 * mesh.X) * torch.cos(2.0 * mesh.Y), 0.8 * torch.cos(2.0 * mesh.Z),
                          -0.6 * torch.sin(mesh.X + mesh.Y)]).contiguous()
        reps = 3 if n <= 256 else 1

        def momentum(order):
            from pyapes_amd.solver.march import momentum_march

            def run():
                U = Field("U", 3, mesh, {"domain": vbcs, "obstacle": None})
                U.set_var_tensor(V3.clone())
                U.apply_bcs()
                ms = timed(lambda: momentum_march(U, nu, dt, steps, cfg, order=order), reps, warm=1) / steps
                assert bool(torch.isfinite(U()).all())
                return ms
            return run

        def three_scalar_marches(order):
            def run():
                phis = []
                for c in range(3):
                    phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
                    phi.set_var_tensor(V3[c:c + 1].clone())
                    phi.apply_bcs()
                    phis.append(phi)
                vel = (V3[0], V3[1], V3[2])
                ms = timed(lambda: [rk_march(phi, vel, nu, dt, steps, cfg, order=order) for phi in phis], reps, warm=1) / steps
                assert all(bool(torch.isfinite(phi()).all()) for phi in phis)
                return ms
            return run

        for order in (1, 3):
            launches = 3 * order
            stage_reads = 3 * (order - 1)
            variants = [("yardstick: three rk_march in three frozen fields", three_scalar_marches(order), {"fastpath": 1}, 5 * launches + stage_reads)]
            if with_momentum:
                variants += [("momentum_march", momentum(order), {"fastpath": 1, "vself": 1}, 4 * launches + stage_reads),
                             ("momentum_march, vself 0", momentum(order), {"fastpath": 1, "vself": 0}, 5 * launches + stage_reads),
                             ("momentum_march, fastpath 0", momentum(order), {"fastpath": 0, "vself": 1}, 5 * launches + stage_reads)]
            rounds = {v[0]: [] for v in variants}
            for _ in range(3):
                for vname, run, opts, _ in variants:
                    for k, v in opts.items():
                        if k != "vself" or with_momentum:
                            ctx.set_option(k, v)
                    rounds[vname].append(run())
            yard = sorted(rounds[variants[0][0]])[1]
            for vname, _, opts, passes in variants:
                ms = sorted(rounds[vname])[1]
                emit(f"order {order} ({steps} steps per call) {n}^3 f32 upwind, {vname} (config 4 BC types)", n ** 3, ms, passes, 4,
                     {"ms_rounds": rounds[vname], "over_yardstick": ms / yard, "options": opts})
        ctx.set_option("fastpath", 1)
        del mesh, V3
        torch.cuda.empty_cache()


def self_rows(q, emit, with_self=True):
    """The self-advected march rk_march(phi, phi) -- div(phi, phi), every launch advected by its own input -- orders 1 and 3,
    beside (a) rk_march with a SEPARATE speed tensor (a frozen speed: the launches read one more stream; central Div with a
    foreign field runs on the generic kernel) and (b) the self-advected march composed step by step from public pieces that
    need no self march: euler_step(phi, copy of phi), c0 * phi0 + c1 * E as torch ops, apply_bcs.  (a) and (b) use nothing
    of the self march (with_self=False: those two alone).  ms per STEP, min and median of 5 marches of 20 steps, every march
    from the same start.  Algorithmic passes of a self step: Euler stage 2, every fused stage 3 -- order 3: 8, order 1: 2."""
    import statistics
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.march import SSP_STAGES, euler_step, rk_march
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    neusym = mixed_bcs([0.0, 0.0, None, None, None, None], ["neumann", "neumann", "symmetry", "symmetry", "symmetry", "symmetry"])
    alldir = mixed_bcs([0.0] * 6, ["dirichlet"] * 6)
    nu, steps, nrep = 1e-3, 20, 5

    def composed(phi, dt, order, cfg):
        for _ in range(steps):
            phi0 = phi()
            euler_step(phi, phi0.clone(), nu, dt, cfg)
            for c0, c1 in SSP_STAGES[order]:
                euler_step(phi, phi().clone(), nu, dt, cfg)
                phi.set_var_tensor(c0 * phi0 + c1 * phi())
                phi.apply_bcs()

    def measure(phi, start, fn):
        ms = []
        for r in range(nrep + 1):          # the first march is the warm-up
            phi.set_var_tensor(start.clone())
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / steps)
        assert bool(torch.isfinite(phi()).all())
        return min(ms[1:]), statistics.median(ms[1:])

    if q:
        sizes = [(128, "single", neusym, "upwind", "config 4 BCs"), (64, "double", alldir, "none", "dirichlet")]
    else:
        sizes = [(256, "single", neusym, "upwind", "config 4 BCs"), (512, "single", neusym, "upwind", "config 4 BCs"),
                 (256, "double", alldir, "none", "dirichlet")]
    for n, dtype, bcs, limiter, bname in sizes:
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", dtype)
        es, f = (8, "f64") if dtype == "double" else (4, "f32")
        cfg = {"div": {"limiter": limiter}}
        sch = "central" if limiter == "none" else limiter
        phi = Field("phi", 1, mesh, {"domain": bcs, "obstacle": None})
        phi.set_var_tensor(torch.exp(-((mesh.X - 0.5) ** 2 + (mesh.Y - 0.5) ** 2 + (mesh.Z - 0.5) ** 2) / 0.02).unsqueeze(0).contiguous())
        phi.apply_bcs()
        start = phi().clone()
        dx = mesh.dx_list[0]
        dt = 0.2 * min(dx * dx / (6 * nu), dx / 1.0)
        for order in (3, 1):
            passes = 2 + 3 * (order - 1)
            tag = f"order {order} ({steps} steps per call) {n}^3 {f} {sch} ({bname})"
            res = {}
            if with_self:
                res["self"] = measure(phi, start, lambda: rk_march(phi, phi, nu, dt, steps, cfg, order=order))
            ut = start.clone()
            res["a"] = measure(phi, start, lambda: rk_march(phi, ut, nu, dt, steps, cfg, order=order))
            del ut
            res["b"] = measure(phi, start, lambda: composed(phi, dt, order, cfg))
            if with_self:
                emit(f"self-advected rk_march {tag}", n ** 3, res["self"][0], passes, es,
                     {"ms_median": res["self"][1], "reps": nrep, "self_over_separate_speed": res["self"][0] / res["a"][0],
                      "self_over_composition": res["self"][0] / res["b"][0]})
            emit(f"(a) rk_march, separate speed tensor {tag}", n ** 3, res["a"][0], passes + order, es,
                 {"ms_median": res["a"][1], "reps": nrep})
            emit(f"(b) self-advected composition (euler_step with a copy as speed + torch combine + apply_bcs) {tag}", n ** 3,
                 res["b"][0], passes + order, es, {"ms_median": res["b"][1], "reps": nrep})
        del phi, mesh, start
        torch.cuda.empty_cache()


def solver_rows(q, emit, sections):
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.fdm import FDM
    from pyapes_amd.solver.ops import Solver
    from pyapes_amd.testing.poisson import poisson_bcs, poisson_rhs_nd
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import homogeneous_bcs, mixed_bcs

    # --- solvers: ms per iteration from fixed-iteration solves ------------------------------------
    def solver_ms(meshf, bcsf, method, K, rhs_fn=None, extra_cfg=None, resident=True, eq=lambda v: FDM().laplacian(1.0, v)):
        os.environ["PYAPES_HIP_RESIDENT"] = "1" if resident else "0"   # read when the mesh's context is created
        mesh = meshf()
        var = Field("p", 1, mesh, {"domain": bcsf, "obstacle": None})
        rhs = rhs_fn(mesh, var) if rhs_fn else torch.randn_like(var())
        cfg = {"method": method, "tol": -1.0, "max_it": K - 1, "report": False}
        cfg.update(extra_cfg or {})
        # one short untimed solve first (same mesh / context): code-object load, scratch allocation
        warm = Field("p", 1, mesh, {"domain": bcsf, "obstacle": None})
        sw = Solver({"fdm": dict(cfg, max_it=3)})
        sw.set_eq(eq(warm) == rhs.clone())
        sw.solve()
        s = Solver({"fdm": cfg})
        s.set_eq(eq(var) == rhs)
        t0 = time.perf_counter()
        rep = s.solve()
        wall = (time.perf_counter() - t0) * 1e3
        from pyapes_amd.hip.context import context_for as _cf
        solver_ms.boxes = _cf(mesh).resident_used()
        return var.last_gpu_ms / rep["itr"], wall / rep["itr"], rep["itr"], mesh.N

    K = 200
    # the sizes pyapes users run (the reference's tests and demos): the whole solve is ONE cooperative launch with
    # the fields in LDS (pa_resident.hip); beside it the launch-per-phase loops it replaces (DESIGN.md "small meshes")
    m2 = lambda nn: (lambda: Mesh(Box[0:1, 0:1], None, [nn, nn], "cuda", "double"))
    m3 = lambda nn: (lambda: Mesh(Box[0:1, 0:1, 0:1], None, [nn, nn, nn], "cuda", "double"))
    mixbc = mixed_bcs([0, 0, 0, 0, 1, 0], ["dirichlet", "neumann"] * 3)
    m1 = lambda nn: (lambda: Mesh(Box[0:1], None, [nn], "cuda", "double"))
    small = [("cg 1-D 101 nodes f64 dirichlet (the reference's 1-D Poisson test: one box, no grid-wide step)", m1(101), poisson_bcs(1), "cg", 100,
              10, poisson_rhs_nd),
             ("bicgstab 1-D 101 nodes f64 dirichlet", m1(101), poisson_bcs(1), "bicgstab", 60, 22, poisson_rhs_nd),
             ("cg 2-D 32x32 f64 dirichlet (one box)", m2(32), poisson_bcs(2), "cg", 100, 10, poisson_rhs_nd),
             ("jacobi 2-D 128x128 f64 dirichlet (config 1)", m2(128), poisson_bcs(2), "jacobi", 1000, 3, poisson_rhs_nd),
             ("cg 2-D 128x128 f64 dirichlet (config 1 inputs)", m2(128), poisson_bcs(2), "cg", 271, 10, poisson_rhs_nd),
             ("bicgstab 2-D 128x128 f64 dirichlet (config 1 inputs)", m2(128), poisson_bcs(2), "bicgstab", 100, 22, poisson_rhs_nd)]
    # the reference's own solver tests at their sizes: x-periodic 101^2 (tests/test_solver.py:164-207) and the
    # axisymmetric 101^2 Poisson problem (tests/test_solver.py:309-358; round 3: the resident solver's lean stencil
    # takes the r rows from an LDS copy of pa_coord_set's table)
    from pyapes_amd.geometry import Cylinder
    from pyapes_amd.testing.poisson import poisson_rz_bcs, poisson_rz_rhs
    from pyapes_amd.variables.bcs import CylinderBoundary
    rzc = poisson_rz_bcs()
    rz_bcs = CylinderBoundary(rl={"bc_type": "neumann", "bc_val": 0.0}, ru={"bc_type": "dirichlet", "bc_val": rzc[1]["bc_val"]},
                              zl={"bc_type": "dirichlet", "bc_val": rzc[2]["bc_val"]},
                              zu={"bc_type": "dirichlet", "bc_val": rzc[3]["bc_val"]})()
    mrz = lambda: Mesh(Cylinder[0:1, 0:1], None, [101, 101], "cuda", "double")
    xper = mixed_bcs([None, None, 0, 0], ["periodic", "periodic", "dirichlet", "dirichlet"])
    small += [("bicgstab 2-D 101x101 f64 x-periodic / y-dirichlet (the reference's test_poisson_2d_mixed_periodic)", m2(101), xper,
               "bicgstab", 100, 22, None),
              ("bicgstab axisymmetric (rz) 101x101 f64 (the reference's test_poisson_rz)", mrz, rz_bcs, "bicgstab", 100, 22,
               poisson_rz_rhs),
              ("cg axisymmetric (rz) 101x101 f64", mrz, rz_bcs, "cg", 100, 10, poisson_rz_rhs)]
    for nn in (32, 64):
        for meth, its, passes in (("jacobi", 200, 3), ("cg", 60, 10), ("bicgstab", 40, 22)):
            small.append((f"{meth} 3-D {nn}^3 f64 dirichlet/neumann faces (BC fill every iteration)", m3(nn), mixbc, meth, its,
                          passes, None))
    for name, meshf, bcs_, meth, its, passes, rfn in (small if "small" in sections else []):
        for res in (True, False):
            torch.manual_seed(0)
            ms, wall, itr, N = solver_ms(meshf, bcs_, meth, its, rfn, resident=res)
            how = f"resident, {solver_ms.boxes} workgroups" if solver_ms.boxes else "launch per phase"
            emit(f"{name} [{how}]", N, ms, passes, 8, {"wall_ms_per_iter": wall, "iters": itr})
    if "small" in sections:
        # a term list with a Div term: the resident kernel evaluates the generic term list on its box (no lean stencil)
        fdm_up = FDM({"div": {"limiter": "upwind", "edge": False}})
        for res in (True, False):
            torch.manual_seed(0)
            ms, wall, itr, N = solver_ms(m3(32), homogeneous_bcs(3, 0.0, "dirichlet"), "bicgstab", 40, lambda m, v: torch.ones_like(v()),
                                         resident=res, eq=lambda v: fdm_up.div(1.0, v) - fdm_up.laplacian(0.05, v))
            how = f"resident, {solver_ms.boxes} workgroups" if solver_ms.boxes else "launch per phase"
            emit(f"bicgstab 3-D 32^3 f64 steady advection-diffusion (upwind Div + Laplacian), dirichlet [{how}]", N, ms, 22, 8,
                 {"wall_ms_per_iter": wall, "iters": itr})
    os.environ["PYAPES_HIP_RESIDENT"] = "1"
    if "big" not in sections:
        return
    # the generic one-cell-per-thread solver kernels (k_jacobi, k_cg_a / k_cg_b, k_bicg_*: "fastpath" 0, launch per phase) at 128^3
    def generic_mesh(dt):
        from pyapes_amd.hip.context import context_for as _cf
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [128, 128, 128], "cuda", dt)
        _cf(mesh).set_option("fastpath", 0)
        return mesh

    for dt, es in (("double", 8), ("single", 4)):
        for meth, its, passes in (("jacobi", 200, 3), ("cg", 100, 10), ("bicgstab", 60, 22)):
            torch.manual_seed(0)
            ms, wall, itr, N = solver_ms(lambda: generic_mesh(dt), mixbc, meth, its, resident=False)
            emit(f"{meth} 3-D 128^3 {'f64' if es == 8 else 'f32'} dirichlet/neumann faces, fastpath 0 (generic kernels)", N, ms, passes, es,
                 {"wall_ms_per_iter": wall, "iters": itr})
    n = 128 if q else 256   # (solver_ms sets the resident switch on every call: the rows below run with it on again)
    ms, wall, itr, N = solver_ms(lambda: Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", "double"),
                                 homogeneous_bcs(3, 0.0, "dirichlet"), "jacobi", K)
    emit(f"jacobi 3-D {n}^3 f64 dirichlet", N, ms, 3, 8, {"wall_ms_per_iter": wall, "iters": itr})
    ms, wall, itr, N = solver_ms(lambda: Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", "double"),
                                 mixed_bcs([0, 0, 0, 0, 1, 0], ["dirichlet", "neumann"] * 3), "bicgstab", 100)
    emit(f"bicgstab 3-D {n}^3 f64 mixed", N, ms, 22, 8, {"wall_ms_per_iter": wall, "iters": itr})
    if not q:
        # round 4: the three solver loops at BASELINE config 3's size (512^3 fp64), Dirichlet and fully periodic -- BiCGSTAB is
        # the method that converges on the periodic problem; passes = the algorithmic count
        per3 = mixed_bcs([None] * 6, ["periodic"] * 6)
        for bname, bcs3 in (("dirichlet", homogeneous_bcs(3, 0.0, "dirichlet")), ("periodic", per3)):
            for meth, its, passes in (("jacobi", 60, 3), ("cg", 60, 10), ("bicgstab", 40, 22)):
                ms, wall, itr, N = solver_ms(lambda: Mesh(Box[0:1, 0:1, 0:1], None, [512, 512, 512], "cuda", "double"), bcs3, meth, its)
                emit(f"{meth} 3-D 512^3 f64 {bname}", N, ms, passes, 8, {"wall_ms_per_iter": wall, "iters": itr})
                torch.cuda.empty_cache()
    def advdiff_ms(n):
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, [n, n, n], "cuda", "double")
        var = Field("p", 1, mesh, {"domain": homogeneous_bcs(3, 0.0, "dirichlet"), "obstacle": None})
        s = Solver({"fdm": {"method": "bicgstab", "tol": -1.0, "max_it": 60, "report": False}})
        fdm = FDM({"div": {"limiter": "upwind", "edge": False}})
        s.set_eq(fdm.div(1.0, var) - fdm.laplacian(0.05, var) == torch.ones_like(var()))
        rep = s.solve()
        return var.last_gpu_ms / rep["itr"], rep["itr"], mesh.N

    ms, itr, N = advdiff_ms(n)
    emit(f"bicgstab 3-D {n}^3 f64 steady advection-diffusion (upwind Div + Laplacian)", N, ms, 22, 8, {"iters": itr})
    m2 = 1024 if q else 4096
    ms, wall, itr, N = solver_ms(lambda: Mesh(Box[0:1, 0:1], None, [m2, m2], "cuda", "double"),
                                 homogeneous_bcs(2, 0.0, "dirichlet"), "cg", 100)
    emit(f"cg 2-D {m2}x{m2} f64 dirichlet (marching kernel k_cg2d from 1.5 M cells on)", N, ms, 10, 8, {"wall_ms_per_iter": wall, "iters": itr})
    # round 3, second session: the Jacobi sweep and the BiCGSTAB phases of large 2-D meshes on the marching kernel too;
    # odd extents (node-based meshes: 2^k + 1) through the PITCH layout
    ms, wall, itr, N = solver_ms(lambda: Mesh(Box[0:1, 0:1], None, [m2, m2], "cuda", "double"),
                                 homogeneous_bcs(2, 0.0, "dirichlet"), "jacobi", 100)
    emit(f"jacobi 2-D {m2}x{m2} f64 dirichlet (k_cg2d)", N, ms, 3, 8, {"wall_ms_per_iter": wall, "iters": itr})
    ms, wall, itr, N = solver_ms(lambda: Mesh(Box[0:1, 0:1], None, [m2, m2], "cuda", "double"),
                                 homogeneous_bcs(2, 0.0, "dirichlet"), "bicgstab", 60)
    emit(f"bicgstab 2-D {m2}x{m2} f64 dirichlet (k_cg2d phases 6 / 8)", N, ms, 22, 8, {"wall_ms_per_iter": wall, "iters": itr})
    n3 = 129 if q else 257
    mixbc3 = mixed_bcs([0, 0, 0, 0, 1, 0], ["dirichlet", "neumann"] * 3)
    for meth, its, passes in (("cg", 100, 10), ("bicgstab", 60, 22)):
        ms, wall, itr, N = solver_ms(lambda: Mesh(Box[0:1, 0:1, 0:1], None, [n3, n3, n3], "cuda", "double"), mixbc3, meth, its)
        emit(f"{meth} 3-D {n3}^3 f64 mixed (odd rows: PITCH layout)", N, ms, passes, 8, {"wall_ms_per_iter": wall, "iters": itr})


if __name__ == "__main__":
    main()
