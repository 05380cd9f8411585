"""-m gpu: the pressure-carrying projection -- ``pa_project_update`` (k_project_update) and ``pa_flow_stats`` (k_flow_stats) at
the C ABI, and ``form=`` of ``project`` / ``ns_step``, ``flow_stats`` and ``ns_march`` of pyapes_amd/solver/projection.py.

The yardstick is tests/projection_ref.py, and the device must give its BITS: the setups, meshes, BC sets, scales and offsets are
those of tests/test_gpu_projection.py (tests/projection_gpu.py has them), with DISTINCT random U, p, phi and nrhs.
``pa_project_update`` is also held against the sequence it replaces, ``pa_project_correct`` and two ``pa_vec_axpy``.  The maxima of ``pa_flow_stats`` are exact; its two sums are
double sums of N non-negative addends in the grid's order, within 2 N 2^-53 relative of the restatement's ``math.fsum``
(tests/test_pressure_host.py has the bound).  ``ns_step(form=...)`` is compared with the CPU chain at a fixed iteration count, to
the suite's solver tolerances; the rest state of DESIGN.md section 4 "Incremental form" must be held in every bit.
"""
import ctypes as C
import math
import warnings

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
from pyapes_amd.solver.march import momentum_step
from pyapes_amd.solver.projection import flow_stats, ns_march, ns_step, project
from pyapes_amd.variables import Field
from pyapes_amd.variables.bcs import mixed_bcs

pytestmark = pytest.mark.gpu

DT, SCALES, TWO_PASSES = PG.DT, PG.SCALES, PG.TWO_PASSES
CHI = 0.37
_ids = G.mesh_id


# ---- pa_project_update ----------------------------------------------------------------------------------------------
def check_update(n, dtype, bcnames, scales=SCALES, offsets=(None,)):
    bad = []
    for bcname in bcnames:
        mesh, bc, om, obcs, U_c, p_c, phi_c, r_c = PG.setup(n, dtype, bcname)
        ctx = context_for(mesh)
        f = G.fresh_field(mesh, bc, U_c)
        ctx.bind_bcs(f(), f.bcs, 0)
        for scale in scales:
            for rot in (False, True):
                want_U, want_p = PR.update(U_c, phi_c, p_c, r_c if rot else None, scale, CHI, om, obcs)
                want_n = PR.update(U_c, phi_c, p_c, r_c if rot else None, scale, CHI, om, obcs, fill=False)[0]
                for k in offsets:
                    tag = (bcname, scale, rot, k)
                    Ud, Ua = PG.dev(U_c, k)
                    pd, pa = PG.dev(p_c[0], k)
                    fd, fa = PG.dev(phi_c[0], k)
                    rd, ra = PG.dev(r_c[0], k)
                    got = ctx.project_update(Ud, fd, scale, pd, rd if rot else None, CHI, f.bcs)
                    if got is not Ud or not same_bits(Ud, want_U) or not same_bits(pd, want_p[0]):
                        bad.append((tag, "fused", same_bits(Ud, want_U), same_bits(pd, want_p[0])))
                    if not same_bits(fd, phi_c[0]) or not same_bits(rd, r_c[0]):
                        bad.append((tag, "phi or nrhs was written"))
                    # the sequence it replaces: the correction and two AXPYs (the product rounded first, as in the kernel)
                    U2, p2 = U_c.cuda(), p_c[0].cuda()
                    ctx.project_correct(U2, fd, scale, f.bcs)
                    ctx.vec_axpy(p2, p2, 1.0, fd)
                    if rot:
                        ctx.vec_axpy(p2, p2, CHI, rd)
                    if not same_bits(U2, Ud) or not same_bits(p2, pd):
                        bad.append((tag, "composed", same_bits(U2, Ud), same_bits(p2, pd)))
                    Ud.copy_(U_c)
                    pd.copy_(p_c[0])
                    ctx.project_update(Ud, fd, scale, pd, rd if rot else None, CHI, None)    # no fill behind the kernel
                    if not same_bits(Ud, want_n) or not same_bits(pd, want_p[0]):
                        bad.append((tag, "no fill", same_bits(Ud, want_n)))
                    for view, alloc in ((Ud, Ua), (pd, pa), (fd, fa), (rd, ra)):
                        if alloc is not None and not guards_intact(alloc, view):
                            bad.append((tag, "a guard was written"))
    return bad


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [[9, 132], [11, 13], [10, 12, 132], [11, 13, 17]], ids=_ids)
def test_update_gives_the_restated_bits_and_those_of_the_composed_calls(n, dtype):
    assert check_update(n, dtype, ("dir", "mix", "xper", "per")) == []


@pytest.mark.parametrize("dtype", ["double", "single"])
def test_update_on_two_passes_of_the_flat_grid(dtype):
    assert check_update(TWO_PASSES, dtype, ("mix",), scales=(1.0 / DT,)) == []


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [[9, 132], [10, 12, 132], [11, 13, 17]], ids=_ids)
def test_update_on_operands_off_16_byte_alignment(n, dtype):
    offsets = (0, 1) if dtype == "double" else (0, 1, 3)
    assert check_update(n, dtype, ("mix", "per"), scales=(-0.75,), offsets=offsets) == []


# ---- pa_flow_stats --------------------------------------------------------------------------------------------------
def stats_differ(got, U_c, om, obcs):
    """what of (rate, div_max, div_sq, ke_sq) misses the restatement: the maxima exactly, the sums within 2 N 2^-53 relative"""
    want = PR.flow_stats(U_c, om, obcs)
    n_div, n_ke = PR.addends(U_c, om, obcs)
    bad = []
    for name, g in zip(("rate", "div_max"), got[:2]):
        if not (g == want[name] or (math.isnan(g) and math.isnan(want[name]))):
            bad.append((name, g, want[name]))
    for name, g, N in (("div_sq", got[2], n_div), ("ke_sq", got[3], n_ke)):
        if not abs(g - want[name]) <= PR.SUM_BOUND * N * want[name]:
            bad.append((name, g, want[name], abs(g - want[name]) / max(want[name], 1e-300), PR.SUM_BOUND * N))
    return bad


def check_stats(n, dtype, bcnames, offsets=(None,), fields=None):
    bad = []
    for bcname in bcnames:
        mesh, bc, om, obcs, U_c, _, _, _ = PG.setup(n, dtype, bcname)
        ctx = context_for(mesh)
        f = G.fresh_field(mesh, bc, U_c)
        ctx.bind_bcs(f(), f.bcs, 0)
        sl = O.interior_slicer(len(n), obcs)
        for name, V in (fields(U_c) if fields else [("random", U_c)]):
            for k in offsets:
                Vd, Va = PG.dev(V, k)
                got = ctx.flow_stats(Vd)
                bad += [(bcname, name, k) + b for b in stats_differ(got, V, om, obcs)]
                dmax = float(ctx.divergence(Vd, 1.0)[sl].abs().max().double())
                if not (got[1] == dmax or (math.isnan(got[1]) and math.isnan(dmax))):
                    bad.append((bcname, name, k, "div_max is not the divergence's", got[1], dmax))
                if not same_bits(Vd, V) or (Va is not None and not guards_intact(Va, Vd)):
                    bad.append((bcname, name, k, "U or a guard was written"))
    return bad


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [[9, 132], [11, 13], [10, 12, 132], [11, 13, 17]], ids=_ids)
def test_flow_stats_against_the_restatement(n, dtype):
    assert check_stats(n, dtype, ("dir", "mix", "xper", "per")) == []


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [[9, 132], [11, 13, 17]], ids=_ids)
def test_flow_stats_on_operands_off_16_byte_alignment(n, dtype):
    offsets = (0, 1) if dtype == "double" else (0, 1, 3)
    assert check_stats(n, dtype, ("mix", "per"), offsets=offsets) == []


def _extremes(U_c):
    """the maximum in the last cell of the last pass, the maximum in cell 0, and the random field itself"""
    small = 0.01 * U_c
    last, first = small.clone(), small.clone()
    last.view(U_c.shape[0], -1)[:, -1] = 50.0
    first.view(U_c.shape[0], -1)[:, 0] = -60.0
    return [("random", U_c), ("last cell", last), ("cell 0", first)]


@pytest.mark.parametrize("dtype", ["double", "single"])
def test_flow_stats_on_two_passes_of_the_flat_grid_and_their_extremes(dtype):
    """533 628 cells: the second pass of the grid-stride loop covers the last 9 340, whose last cell holds the maximum once;
    fully periodic faces make that cell a member of the interior set"""
    assert check_stats(TWO_PASSES, dtype, ("per",), fields=_extremes) == []
    assert check_stats(TWO_PASSES, dtype, ("mix",), offsets=(1,)) == []


@pytest.mark.parametrize("dtype", ["double", "single"])
def test_flow_stats_of_a_zero_field_and_of_a_nan(dtype):
    n = [11, 13, 17]
    mesh, bc, om, obcs, U_c, _, _, _ = PG.setup(n, dtype, "dir")
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, U_c)
    ctx.bind_bcs(f(), f.bcs, 0)
    got = ctx.flow_stats(torch.zeros_like(U_c).cuda())
    assert got == (0.0, 0.0, 0.0, 0.0) and not any(math.copysign(1.0, v) < 0 for v in got)
    clean = ctx.flow_stats(U_c.cuda())
    V = U_c.clone()
    V[2, 0, 5, 7] = float("nan")            # the last component on face xl: off the interior set, and no interior stencil reads it
    got = ctx.flow_stats(V.cuda())
    assert math.isnan(got[0]) and got[1] == clean[1] and math.isfinite(got[2]) and math.isnan(got[3])
    V = U_c.clone()
    V[1, 5, 5, 7] = float("nan")            # inside: the divergence of its neighbours along axis 1 reads it
    got = ctx.flow_stats(V.cuda())
    assert all(math.isnan(v) for v in got)


@pytest.mark.parametrize("n,dtype", [([11, 13], "double"), ([10, 12, 132], "single")], ids=_ids)
def test_flow_stats_entry_point(n, dtype):
    """``flow_stats(U)``: the BC fill first, the four numbers; with ``dt`` the three derived ones, formed in double"""
    for bcname in ("mix", "per"):
        mesh, bc, om, obcs, U_c, _, _, _ = PG.setup(n, dtype, bcname)
        filled = O.bc_fill(U_c.clone(), obcs)
        f = G.fresh_field(mesh, bc, U_c)
        got = flow_stats(f)
        assert list(got) == ["rate", "div_max", "div_sq", "ke_sq"] and same_bits(f(), filled)
        assert stats_differ(tuple(got.values()), filled, om, obcs) == []
        more = flow_stats(G.fresh_field(mesh, bc, U_c), DT)
        vol = math.prod(float(h) for h in mesh.dx_list)
        assert list(more) == ["rate", "div_max", "div_sq", "ke_sq", "cfl", "div_l2", "ke"]
        assert all(more[k] == got[k] for k in got)
        assert more["cfl"] == DT * got["rate"] and more["div_l2"] == math.sqrt(got["div_sq"] * vol)
        assert more["ke"] == 0.5 * got["ke_sq"] * vol


# ---- ns_step(form=...) ----------------------------------------------------------------------------------------------
NU, STEP_DT, RHO = 1e-3, 2e-3, 1.3
SOLVER = {"fdm": {"method": "cg", "tol": -1.0, "max_it": 4, "report": False}}


def _source(U_c):
    g = torch.Generator().manual_seed(23)
    return (3.0 * torch.randn(U_c.shape, generator=g, dtype=torch.float64)).to(U_c.dtype)


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("form", ["incremental", "rotational"])
def test_ns_step_against_the_cpu_chain(form, dtype):
    """a fixed iteration count (tol -1, max_it 4): U, p and itr against the seven statements on the CPU, with and without a
    source; the suite's solver tolerances"""
    mesh, om, ubc, pbc, ubcs, pcfg, U_c, p_c = PG.project_case("walled", dtype)
    tol = 1e-10 if dtype == "double" else 1e-5
    for S in (None, _source(U_c)):
        U_w, p_w, rep_w = PR.ns_step(U_c, p_c, NU, STEP_DT, RHO, om, ubcs, pcfg, form, -1.0, 4, "upwind", 3, S)
        Uf, pf = G.fresh_field(mesh, ubc, U_c, time=True), PG.pressure(mesh, pbc, p_c)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rep = ns_step(Uf, pf, NU, STEP_DT, G.config("upwind"), 3, rho=RHO, solver=SOLVER, form=form,
                          source=None if S is None else S.cuda())
        eu, ep = rel_err(Uf().cpu(), U_w), rel_err(pf().cpu(), p_w)
        print(f"ns_step {form} {dtype} source {S is not None}: itr {rep['itr']} / {rep_w['itr']}, rel err U {eu:.3e}, p {ep:.3e}")
        assert rep["itr"] == rep_w["itr"] == 5
        assert eu <= tol and ep <= tol
        assert abs(float(Uf.t) - (1.5 + STEP_DT)) <= 1e-12
        assert rel_err(U_w, U_c) > 1e-3 and rel_err(p_w, p_c) > 1e-3          # the step did something to both
    # the two forms differ, and both differ from Chorin's (the CPU chain: what the device was just held against)
    others = [PR.ns_step(U_c, p_c, NU, STEP_DT, RHO, om, ubcs, pcfg, g, -1.0, 4)[1] for g in PR.FORMS if g != form]
    assert all(rel_err(o, p_w) > 1e-6 for o in others)


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("form", ["incremental", "rotational"])
def test_a_step_on_a_used_mesh_equals_a_step_on_a_fresh_one(form, dtype):
    """three steps on one mesh -- with a source, without, with -- against every step redone on a mesh that has seen nothing,
    from the previous state, bit for bit: neither phi nor the work tensors S / src / nrhs carry state"""
    mesh, om, ubc, pbc, ubcs, pcfg, U_c, p_c = PG.project_case("walled", dtype)
    cfg = G.config("upwind")
    srcs = [_source(U_c).cuda(), None, (0.5 * _source(U_c)).cuda()]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Uf, pf = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, p_c)
        states = []
        for step in range(3):
            assert ns_step(Uf, pf, NU, STEP_DT, cfg, 3, rho=RHO, solver=SOLVER, form=form, source=srcs[step])["itr"] == 5
            states.append((Uf().clone(), pf().clone()))
        assert pf._increment.mesh is mesh and pf._increment is not pf
        prev = (U_c.cuda(), p_c.cuda())
        for step in range(3):
            fresh = Mesh(G.box(3), None, list(U_c.shape[1:]), "cuda", dtype)
            Uh, ph = G.fresh_field(fresh, ubc, prev[0]), PG.pressure(fresh, pbc, prev[1].clone())
            phi = Field("phi", 1, fresh, {"domain": mixed_bcs([0.0] * 6, ["neumann", "dirichlet"] + ["neumann"] * 4), "obstacle": None})
            phi.set_var_tensor(torch.full_like(ph(), 7.0))                  # a caller's phi, with content: it is zeroed
            ns_step(Uh, ph, NU, STEP_DT, cfg, 3, rho=RHO, solver=SOLVER, form=form, source=srcs[step], phi=phi)
            assert same_bits(Uh(), states[step][0]), (step, same_bits(Uh(), states[step][0]))
            assert same_bits(ph(), states[step][1]), (step, same_bits(ph(), states[step][1]))
            assert not hasattr(ph, "_increment")
            prev = states[step]


@pytest.mark.parametrize("dtype", ["double", "single"])
def test_form_chorin_is_the_path_as_it_was(dtype):
    """``form="chorin"`` and no ``form`` at all: the bits of ``momentum_step`` then ``project``, on ``ns_step`` and ``project``"""
    mesh, om, ubc, pbc, ubcs, pcfg, U_c, p_c = PG.project_case("walled", dtype)
    cfg = G.config("upwind")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Ug, pg = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, p_c)
        momentum_step(Ug, NU, STEP_DT, cfg, 3)
        mid = Ug().clone()
        project(Ug, pg, STEP_DT, RHO, SOLVER)
        for kw in ({}, {"form": "chorin"}):
            Uf, pf = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, p_c)
            ns_step(Uf, pf, NU, STEP_DT, cfg, 3, rho=RHO, solver=SOLVER, **kw)
            assert same_bits(Uf(), Ug()) and same_bits(pf(), pg()), kw
            assert not hasattr(pf, "_increment")
        Uf, pf = G.fresh_field(mesh, ubc, mid), PG.pressure(mesh, pbc, p_c)
        project(Uf, pf, STEP_DT, RHO, SOLVER, "chorin")
        assert same_bits(Uf(), Ug()) and same_bits(pf(), pg())
        # project(form="incremental") is statements 4 - 7 on its own
        Uf, pf = G.fresh_field(mesh, ubc, mid), PG.pressure(mesh, pbc, p_c)
        rep = project(Uf, pf, STEP_DT, RHO, SOLVER, "incremental")
        Us = O.bc_fill(mid.cpu().clone(), ubcs)
        nrhs = PR.divergence(Us, om, ubcs, -(RHO / STEP_DT))
        phi, rep_w = PR.cg(om, PR.increment_cfg(pcfg), nrhs, torch.zeros_like(p_c), -1.0, 4)
        U_w, q = PR.update(Us, phi, p_c, None, STEP_DT / RHO, 0.0, om, ubcs)
        p_w = O.bc_fill(q, O.make_bcs(om, pcfg))
        tol = 1e-10 if dtype == "double" else 1e-5
        assert rep["itr"] == rep_w["itr"] == 5
        assert rel_err(Uf().cpu(), U_w) <= tol and rel_err(pf().cpu(), p_w) <= tol


# ---- the rest state -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [[17, 21], [10, 12, 20]], ids=_ids)
@pytest.mark.parametrize("form", ["incremental", "rotational"])
def test_the_rest_state_is_held_in_every_bit(form, n, dtype):
    """U = 0 between walls under the body force that p0 balances (projection_ref.rest_case): after three steps with the
    default solver U is +0 in every bit and p has p0's bits.  The right-hand side of every solve is a zero: CG returns after
    its first iteration (0 / 0 -> 0: family A of tests/degenerate_cases.py, ``zero_start_returned``)"""
    nd = len(n)
    om, ubcs, (uvals, utypes), (pcfg, ptypes), U0, p0, S = PR.rest_case(n, dtype)
    mesh = Mesh(G.box(nd), None, list(n), "cuda", dtype)
    Uf = G.fresh_field(mesh, {"domain": mixed_bcs(uvals, utypes), "obstacle": None}, U0, time=True)
    pf = PG.pressure(mesh, {"domain": mixed_bcs([0.0] * (2 * nd), ptypes), "obstacle": None}, p0)
    Sd = S.cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for step in range(PR.REST_STEPS):
            rep = ns_step(Uf, pf, PR.REST_NU, PR.REST_DT, None, 3, rho=PR.REST_RHO, source=Sd, form=form)
            assert rep["itr"] == 1, (step, rep)
    assert same_bits(Uf(), torch.zeros_like(U0))
    assert same_bits(pf(), p0)
    assert float(p0.abs().max()) > 0.9 and float(S.abs().max()) > 0.5
    st = flow_stats(Uf, PR.REST_DT)
    assert st["rate"] == 0.0 and st["div_max"] == 0.0 and st["ke"] == 0.0


# ---- ns_march -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["double", "single"])
def test_ns_march_is_a_loop_of_ns_step(dtype):
    mesh, om, ubc, pbc, ubcs, pcfg, U_c, p_c = PG.project_case("walled", dtype)
    cfg = G.config("upwind")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Uf, pf = G.fresh_field(mesh, ubc, U_c, time=True), PG.pressure(mesh, pbc, p_c)
        out = ns_march(Uf, pf, NU, STEP_DT, 3, cfg, 3, rho=RHO, solver=SOLVER)
        Ug, pg = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, p_c)
        reps = [ns_step(Ug, pg, NU, STEP_DT, cfg, 3, rho=RHO, solver=SOLVER, form="incremental") for _ in range(3)]
    assert same_bits(Uf(), Ug()) and same_bits(pf(), pg())
    assert out == {"steps": 3, "t": sum([STEP_DT] * 3), "dt": [STEP_DT] * 3, "itr": [r["itr"] for r in reps],
                   "converge": [r["converge"] for r in reps]}
    assert abs(float(Uf.t) - (1.5 + 3 * STEP_DT)) <= 1e-12


@pytest.mark.parametrize("dtype", ["double", "single"])
def test_ns_march_caps_every_step_by_the_cfl_rate(dtype):
    """dt_k = min(dt, cfl / rate_k), rate_k the restatement's of the BC-filled state before step k.  The rates of this flow fall from
    64 to 42 over four steps (CPU chain: 64.2, 62.3, 52.4, 41.7), so cfl = 57 dt caps the first steps and not the last"""
    mesh, om, ubc, pbc, ubcs, pcfg, U_c, p_c = PG.project_case("walled", dtype)
    cfg = G.config("upwind")
    cfl = 57.0 * STEP_DT
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Uf, pf = G.fresh_field(mesh, ubc, U_c, time=True), PG.pressure(mesh, pbc, p_c)
        out = ns_march(Uf, pf, NU, STEP_DT, 4, cfg, 3, rho=RHO, solver=SOLVER, form="rotational", cfl=cfl)
        Ug, pg = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, p_c)
        want = []
        for k in range(4):
            Ug.apply_bcs()                                                   # as flow_stats does in front of its pass
            rate = PR.flow_stats(Ug().cpu(), om, ubcs)["rate"]
            want.append(min(STEP_DT, cfl / rate))
            ns_step(Ug, pg, NU, want[-1], cfg, 3, rho=RHO, solver=SOLVER, form="rotational")
    print(f"ns_march cfl {dtype}: dt {out['dt']}")
    assert out["dt"] == want and out["steps"] == 4 and out["t"] == sum(want)
    capped = [d < STEP_DT for d in want]
    assert any(capped) and not all(capped), want
    assert same_bits(Uf(), Ug()) and same_bits(pf(), pg())
    assert abs(float(Uf.t) - (1.5 + sum(want))) <= 1e-12


def test_ns_march_names_the_step_whose_rate_is_not_finite():
    mesh, om, ubc, pbc, ubcs, pcfg, U_c, p_c = PG.project_case("walled", "double")
    V = U_c.clone()
    V[1, 5, 6, 7] = float("nan")
    Uf, pf = G.fresh_field(mesh, ubc, V), PG.pressure(mesh, pbc, p_c)
    with pytest.raises(RuntimeError, match="step 0"):
        ns_march(Uf, pf, NU, STEP_DT, 2, G.config("upwind"), 3, solver=SOLVER, cfl=0.5)
    assert same_bits(pf(), p_c)                                              # refused before the step was taken
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Ug, pg = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, p_c)
        assert ns_march(Ug, pg, NU, STEP_DT, 1, G.config("upwind"), 3, solver=SOLVER, cfl=0.5)["steps"] == 1


# ---- the launch log -------------------------------------------------------------------------------------------------
def log_case():
    mesh, om, ubc, pbc, ubcs, pcfg, U_c, p_c = PG.project_case("walled", "double")
    Uf, pf = G.fresh_field(mesh, ubc, U_c), PG.pressure(mesh, pbc, p_c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for form in ("incremental", "incremental", "rotational"):
            ns_step(Uf, pf, NU, STEP_DT, G.config("upwind"), 3, rho=RHO, solver=SOLVER, form=form)
        flow_stats(Uf)


def test_the_launches_appear_in_the_launch_log():
    """per step of the new forms: statement 2's out-of-place correction and ONE k_project_update; no in-place correction"""
    code = ("import torch\nimport test_gpu_pressure as T\n"
            "sys.stderr.write('CASE log\\n'); sys.stderr.flush()\n"
            "T.log_case()\ntorch.cuda.synchronize(); sys.stderr.flush()\n")
    keep = lambda ln: "k_project_update" in ln or "k_project_correct" in ln or "k_flow_stats" in ln
    lines = G.case_log(G.child(code), keep)["log"]
    ncell = 12 * 20 * 36
    correct = "[pyapes_hip] k_project_correct: generic kernel, %d cells" % ncell
    update = "[pyapes_hip] k_project_update: generic kernel, %d cells" % ncell
    assert lines == [correct, update, correct, update, correct,
                     "[pyapes_hip] k_project_update (rotational): generic kernel, %d cells" % ncell,
                     "[pyapes_hip] k_flow_stats: generic kernel, %d cells" % ncell], lines


# ---- errors ---------------------------------------------------------------------------------------------------------
def test_c_abi_errors_leave_the_context_usable():
    n, dtype = [10, 12, 132], "double"
    _, bc, om, obcs, U_c, p_c, phi_c, r_c = PG.setup(n, dtype, "mix")
    mesh = Mesh(G.box(3), None, list(n), "cuda", dtype)   # a context of its own
    ctx = context_for(mesh)
    f = G.fresh_field(mesh, bc, U_c)
    lib, h = ctx.lib, ctx.h
    ncell = U_c[0].numel()
    want_U, want_p = PR.update(U_c, phi_c, p_c, r_c, 0.5, CHI, om, obcs)

    def good():
        ctx.bind_bcs(f(), f.bcs, 0)
        Ud, pd = U_c.cuda(), p_c[0].cuda()
        ctx.project_update(Ud, phi_c[0].cuda(), 0.5, pd, r_c[0].cuda(), CHI, f.bcs)
        assert same_bits(Ud, want_U) and same_bits(pd, want_p[0])
        assert stats_differ(ctx.flow_stats(U_c.cuda()), U_c, om, obcs) == []

    def code_of(call):
        with pytest.raises(PaError) as ei:
            call()
        assert str(ei.value)
        return ei.value.code

    good()
    U, p, phi, r = U_c.cuda(), p_c[0].cuda(), phi_c[0].cuda(), r_c[0].cuda()
    res = (C.c_double * 4)()
    bv = (L.PaBcValues * 3)()
    for c in range(3):
        bv[c] = ctx.bc_values(f(), f.bcs, c)[0]
    for ncomp in (2, 1, 4, 0):
        assert lib.pa_project_update(h, G.ptr(U), ncomp, G.ptr(phi), 1.0, G.ptr(p), None, 0.0, bv) == L.PA_E_ARG
        assert lib.pa_flow_stats(h, G.ptr(U), ncomp, res) == L.PA_E_ARG
    for args in ((None, phi, p), (U, None, p), (U, phi, None)):
        assert lib.pa_project_update(h, G.ptr(args[0]), 3, G.ptr(args[1]), 1.0, G.ptr(args[2]), None, 0.0, bv) == L.PA_E_ARG
    assert lib.pa_flow_stats(h, None, 3, res) == L.PA_E_ARG and lib.pa_flow_stats(h, G.ptr(U), 3, None) == L.PA_E_ARG
    assert same_bits(U, U_c) and same_bits(p, p_c[0])
    good()
    # overlaps: phi on U, p or nrhs; p on U or nrhs; nrhs on U
    inside = [U[0], U[2], U.reshape(-1)[5:5 + ncell].view(p.shape)]
    for comp in inside:
        assert code_of(lambda: ctx.project_update(U, comp, 1.0, p, r, CHI, f.bcs)) == L.PA_E_ARG
        assert code_of(lambda: ctx.project_update(U, phi, 1.0, comp, r, CHI, f.bcs)) == L.PA_E_ARG
        assert code_of(lambda: ctx.project_update(U, phi, 1.0, p, comp, CHI, f.bcs)) == L.PA_E_ARG
    pair = torch.empty(ncell + 16, dtype=U.dtype, device="cuda")
    a, b = pair[:ncell].view(p.shape), pair[16:].view(p.shape)                     # two scalar views, 128 bytes apart
    for x, y in ((a, b), (b, a), (a, a)):
        assert code_of(lambda: ctx.project_update(U, x, 1.0, y, None, 0.0, None)) == L.PA_E_ARG       # phi on p
        assert code_of(lambda: ctx.project_update(U, x, 1.0, p, y, CHI, None)) == L.PA_E_ARG          # phi on nrhs
        assert code_of(lambda: ctx.project_update(U, phi, 1.0, x, y, CHI, None)) == L.PA_E_ARG        # p on nrhs
    assert same_bits(U, U_c) and same_bits(p, p_c[0])
    good()
    # a BC face array inside a buffer of the call
    arr_vals = [None if v is None else [v, v, v] for v in PG.BCS["mix"][0]]
    for buf, name in ((U, "U"), (phi, "phi"), (p, "p"), (r, "nrhs")):
        vals = [None if v is None else list(v) for v in arr_vals]
        vals[0][2] = buf.reshape(-1)[7:7 + n[1] * n[2]]                             # face "xl" of component 2
        fb = Field("U", 3, mesh, {"domain": mixed_bcs(vals, PG.BCS["mix"][1]), "obstacle": None})
        assert code_of(lambda: ctx.project_update(U, phi, 1.0, p, r, CHI, fb.bcs)) == L.PA_E_ARG, name
    good()
    # a live stepwise solve: PA_E_STATE, and after its abort the calls are good again
    var = Field("p", 1, mesh, {"domain": mixed_bcs([0.0] * 6, ["dirichlet"] * 6), "obstacle": None})
    rhs = torch.rand((1, *n), dtype=torch.float64).cuda()
    ctx.bind_bcs(var(), var.bcs, 0)
    ctx.set_terms([{"kind": L.OP_LAPLACIAN, "sign": -1.0, "coeff": 1.0}])
    ctx.cg_begin(var()[0], rhs[0], 1e-30, 1000)
    assert code_of(lambda: ctx.project_update(U, phi, 1.0, p, None, 0.0, None)) == L.PA_E_STATE
    assert code_of(lambda: ctx.flow_stats(U)) == L.PA_E_STATE
    ctx.cg_abort()
    assert same_bits(U, U_c) and same_bits(p, p_c[0])
    good()
    # a 1-D mesh, an axisymmetric mesh: PA_E_ARG; a slab: PA_E_STATE
    line = Mesh(G.box(1), None, [33], "cuda", "double")
    l0, l1, l2 = (torch.zeros((1, 33), dtype=torch.float64, device="cuda") for _ in range(3))
    assert code_of(lambda: context_for(line).project_update(l0, l1[0], 1.0, l2[0])) == L.PA_E_ARG
    assert code_of(lambda: context_for(line).flow_stats(l0)) == L.PA_E_ARG
    cyl = Mesh(Cylinder[0:1, 0:1], None, [16, 16], "cuda", "double")
    c0 = torch.zeros((2, 16, 16), dtype=torch.float64, device="cuda")
    c1, c2 = (torch.zeros((16, 16), dtype=torch.float64, device="cuda") for _ in range(2))
    assert code_of(lambda: context_for(cyl).project_update(c0, c1, 1.0, c2)) == L.PA_E_ARG
    assert code_of(lambda: context_for(cyl).flow_stats(c0)) == L.PA_E_ARG
    slab = Mesh(Box[0:1, 0:1, 0:1], None, [21, 19, 34], "cuda", "double", slab=(0, 2))
    s0 = torch.zeros((3, *slab.nx), dtype=torch.float64, device="cuda")
    s1, s2 = (torch.zeros(tuple(slab.nx), dtype=torch.float64, device="cuda") for _ in range(2))
    assert code_of(lambda: context_for(slab).project_update(s0, s1, 1.0, s2)) == L.PA_E_STATE
    assert code_of(lambda: context_for(slab).flow_stats(s0)) == L.PA_E_STATE
    good()
    # and an ordinary step on the same context still works
    Uf = G.fresh_field(mesh, bc, U_c)
    pf = PG.pressure(mesh, {"domain": mixed_bcs([0.0] * 6, ["dirichlet"] * 6), "obstacle": None}, torch.zeros_like(p_c))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert project(Uf, pf, 0.01, 1.0, {"fdm": {"method": "cg", "tol": -1.0, "max_it": 2, "report": False}}, "incremental")["itr"] == 3
