"""No GPU: the pressure-carrying projection step and the flow diagnostics restated on the CPU (tests/projection_ref.py) against
independent float64 formulas, the well-balanced property of the incremental forms on the CPU chain -- and its absence in
Chorin's form --, the determinacy of the four diagnostics, and the argument checks of ``form=`` / ``phi=`` / ``flow_stats`` /
``ns_march`` (pyapes_amd/solver/projection.py), which fire before a device is touched.

The rest state (DESIGN.md section 4 "Incremental form").  A fluid at rest, U = 0 between walls, under the body force
S = grad(p0) / rho with p = p0: the exact solution stays at rest.  The incremental forms form S_c - (1 / rho) grad_c(p) with the
very operations S was made of, an exact zero; the predictor then leaves U = +0, the right-hand side of the solve is a zero, CG
returns phi = +0 after its first iteration (0/0 -> 0, family A of tests/degenerate_cases.py), and p + phi is p.  Chorin's form
accelerates the fluid by dt S and projects with the approximate projection, which leaves sin^2(k h / 2) of every mode's
divergence: measured on the 17 x 21 case below after three steps, max |U| = 1.479e-3 and max |p - p0| = 2.29e-2, in fp64 and fp32.
"""
import inspect
import math

import numpy as np
import pytest
import torch

import projection_ref as PR
import pyapes_oracle as O
from projection_ref import MIXED_TYPES, cpu_field as _cpu_field, eps_of, interior_mask, smooth_vector
from pyapes_amd.solver import march as M
from pyapes_amd.solver import projection as P

INT_OF = {torch.float64: torch.int64, torch.float32: torch.int32}


def bits(t):
    return t.contiguous().view(INT_OF[t.dtype])


def _mixed(n, dtype):
    nd = len(n)
    om = O.OMesh([0.0] * nd, [1.0, 1.5, 0.75][:nd], list(n), dtype)
    types = MIXED_TYPES[-2 * nd:] if nd == 2 else MIXED_TYPES
    vals = [None if t in ("symmetry", "periodic") else 0.25 for t in types]
    return om, O.make_bcs(om, O.mixed_cfg(vals, types, O.FACES[:2 * nd]))


# ---- the restatement against independent formulas -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [[11, 13], [7, 9, 12]], ids=["2d", "3d"])
def test_restatement_against_a_float64_formula(n, dtype):
    """numpy, float64, the textbook expressions.

    update.  U is projection_ref.correct with phi for p (its bound, tests/test_projection_host.py: 6 eps on the operands).
    p + phi + chi nrhs: every operand is rounded to the dtype, chi is rounded, the product is rounded, and each of the two sums
    rounds a partial sum no larger than the sum of the magnitudes: at most 4 roundings of eps / 2 on the way of any operand,
    2 eps to first order; 4 eps (|p| + |phi| + |chi| |nrhs|) leaves room for the second-order terms.

    flow_stats.  rate: per axis the operand, q_a and the product are rounded, then up to d sums: (3 + d) / 2 eps to first
    order, bound (3 + d) eps times the value; the maximum of two fields differs by at most the largest difference.  div_max: the
    divergence's bound, 6 eps sum_a (|U_a[+1]| + |U_a[-1]|) / (2 dx_a), at its largest.  ke_sq: operand twice and the square,
    1.5 eps to first order, bound 3 eps relative (all addends are non-negative; the fsum adds nothing).  div_sq: with
    |s - s64| <= b per cell, |s^2 - s64^2| <= b (2 |s64| + b), and the square's own rounding eps / 2 s^2."""
    nd = len(n)
    om, bcs = _mixed(n, dtype)
    U64, p64 = smooth_vector(om)
    phi64 = 0.01 * np.roll(p64, 2, 0) - 0.003
    r64 = 3.0 * np.roll(p64, 1, -1) + 0.5
    U = torch.from_numpy(U64).to(om.dtype)
    p, phi, nrhs = (torch.from_numpy(x).to(om.dtype).unsqueeze(0) for x in (p64, phi64, r64))
    dx = [float(om.dx[a]) for a in range(nd)]
    eps = eps_of(om.dtype)
    inside = interior_mask(om, bcs)
    for scale, chi in ((1.0, 0.0), (1.0 / 0.003, 5e-5), (-0.75, -2.0)):
        for with_r in (False, True):
            Un, q = PR.update(U, phi, p, nrhs if with_r else None, scale, chi, om, bcs, fill=False)
            assert torch.equal(Un, PR.correct(U, phi, om, bcs, scale, fill=False))
            want = p64 + phi64 + (chi * r64 if with_r else 0.0)
            bound = 4.0 * eps * (np.abs(p64) + np.abs(phi64) + (abs(chi) * np.abs(r64) if with_r else 0.0))
            assert q.shape == p.shape and q.dtype == om.dtype
            assert np.all(np.abs(q[0].double().numpy() - want) <= bound), (scale, chi, with_r)
            for c in range(nd):
                grad = (np.roll(phi64, -1, c) - np.roll(phi64, 1, c)) / (2.0 * dx[c])
                gb = (np.abs(np.roll(phi64, -1, c)) + np.abs(np.roll(phi64, 1, c))) / (2.0 * dx[c])
                tol = 6.0 * eps * (abs(scale) * gb + np.abs(U64[c]))
                assert np.all(np.abs(Un[c].double().numpy() - (U64[c] - scale * grad))[inside] <= tol[inside]), (scale, c)
        # the fill behind the update is the oracle's, and p gets none
        Uf, qf = PR.update(U, phi, p, nrhs, scale, chi, om, bcs)
        assert torch.equal(Uf, O.bc_fill(PR.update(U, phi, p, nrhs, scale, chi, om, bcs, fill=False)[0], bcs)) and torch.equal(qf, q)
    got = PR.flow_stats(U, om, bcs)
    rate64 = sum(np.abs(U64[a]) / dx[a] for a in range(nd))
    assert abs(got["rate"] - rate64.max()) <= (3 + nd) * eps * rate64.max()
    div64 = sum((np.roll(U64[a], -1, a) - np.roll(U64[a], 1, a)) / (2.0 * dx[a]) for a in range(nd))
    b = 6.0 * eps * sum((np.abs(np.roll(U64[a], -1, a)) + np.abs(np.roll(U64[a], 1, a))) / (2.0 * dx[a]) for a in range(nd))
    assert abs(got["div_max"] - np.abs(div64[inside]).max()) <= b[inside].max()
    sq_bound = (b * (2.0 * np.abs(div64) + b) + eps * (np.abs(div64) + b) ** 2)[inside]
    assert abs(got["div_sq"] - math.fsum((div64[inside] ** 2).tolist())) <= math.fsum(sq_bound.tolist())
    ke64 = math.fsum((U64 ** 2).reshape(-1).tolist())
    assert abs(got["ke_sq"] - ke64) <= 3.0 * eps * ke64
    assert PR.addends(U, om, bcs) == (int(inside.sum()), U.numel())
    assert got["div_max"] > 0.1 and got["rate"] > 1.0


def test_the_restatement_rounds_every_operation_in_the_dtype():
    """fp32: the restated pressure update and rate are NOT the float64 formulas rounded once (they would be, were an operation
    carried out in double); the product with chi is rounded before the sum, and chi itself once"""
    om = O.OMesh([0.0, 0.0], [1.0, 1.0], [11, 13], "single")
    bcs = O.make_bcs(om, O.mixed_cfg([None] * 4, ["periodic"] * 4, O.FACES[:4]))
    g = torch.Generator().manual_seed(3)
    U = torch.randn((2, 11, 13), generator=g, dtype=torch.float64).to(torch.float32)
    p, phi, r = (torch.randn((1, 11, 13), generator=g, dtype=torch.float64).to(torch.float32) for _ in range(3))
    chi = 0.37
    _, q = PR.update(U, phi, p, r, 1.0, chi, om, bcs)
    t = torch.tensor(chi, dtype=torch.float32) * r
    assert torch.equal(q, (p + phi) + t)
    once = (p.double() + phi.double() + chi * r.double()).float()
    assert not torch.equal(q, once)
    assert torch.equal(PR.update(U, phi, p, None, 1.0, chi, om, bcs)[1], p + phi)
    q0, q1 = (torch.tensor(1.0 / float(om.dx[a]), dtype=torch.float64).float() for a in range(2))
    s = (torch.zeros_like(U[0]) + U[0].abs() * q0) + U[1].abs() * q1
    assert torch.equal(PR.rate_field(U, om), s)
    once = (U[0].abs().double() / float(om.dx[0]) + U[1].abs().double() / float(om.dx[1])).float()
    assert not torch.equal(s, once)
    st = PR.flow_stats(U, om, bcs)
    d = PR.divergence(U, om, bcs)[0]
    assert st["div_sq"] == math.fsum((d * d).double().flatten().tolist())          # the square in fp32, the sum in double
    assert st["div_sq"] != math.fsum((d.double() * d.double()).flatten().tolist())
    assert st["ke_sq"] == math.fsum((U * U).double().flatten().tolist())


# ---- the rest state -------------------------------------------------------------------------------------------------
def _three_steps(form, dtype, n=(17, 21)):
    om, ubcs, _, (pcfg, _), U, p0, S = PR.rest_case(list(n), dtype)
    p, itr = p0.clone(), []
    for _ in range(PR.REST_STEPS):
        U, p, rep = PR.ns_step(U, p, PR.REST_NU, PR.REST_DT, PR.REST_RHO, om, ubcs, pcfg, form, 1e-6, 1000, S=S)
        itr.append(rep["itr"])
    return U, p, p0, itr


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("form", ["incremental", "rotational"])
def test_the_carried_pressure_holds_the_rest_state_bit_for_bit(form, dtype):
    U, p, p0, itr = _three_steps(form, dtype)
    assert bool((bits(U) == 0).all())                    # +0 in every bit
    assert torch.equal(bits(p), bits(p0))
    assert itr == [1, 1, 1]
    assert float(p0.abs().max()) > 0.9                   # and the balanced pressure is not a trivial one


@pytest.mark.parametrize("dtype", ["double", "single"])
def test_chorins_form_does_not_hold_the_rest_state(dtype):
    """the same three steps on the restated chain (measured: 1.479e-3 and 2.29e-2 in both precisions; the floors leave a
    factor 10)"""
    U, p, p0, itr = _three_steps("chorin", dtype)
    print(f"rest state, chorin, {dtype}: max |U| {float(U.abs().max()):.4e}, max |p - p0| {float((p - p0).abs().max()):.4e}, itr {itr}")
    assert float(U.abs().max()) > 1e-4
    assert float((p - p0).abs().max()) > 1e-3


# ---- determinacy of the diagnostics ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["double", "single"])
def test_flow_stats_do_not_depend_on_the_order_of_the_cells(dtype):
    """the maxima are the same under any permutation of the cells, exactly; a double sum of the N non-negative addends in
    any order -- forwards, backwards, permuted, torch's pairwise -- lies within 2 N 2^-53 relative of the ``math.fsum``
    (every partial sum is at most the total, N - 1 roundings of 2^-53 relative each, the fsum's own one on top)"""
    om, bcs = _mixed([7, 9, 12], dtype)
    U = torch.from_numpy(smooth_vector(om)[0]).to(om.dtype)
    st = PR.flow_stats(U, om, bcs)
    sl = O.interior_slicer(3, bcs)
    s = PR.rate_field(U, om).double().flatten()
    d = PR.divergence(U, om, bcs)[0][sl]
    dabs = d.abs().double().flatten()
    dsq = (d * d).double().flatten()
    ke = (U * U).double().flatten()
    assert PR.addends(U, om, bcs) == (dsq.numel(), ke.numel())
    gen = torch.Generator().manual_seed(11)
    for trial in range(4):
        for name, v in (("rate", s), ("div_max", dabs)):
            perm = torch.randperm(v.numel(), generator=gen)
            m = 0.0
            for x in v[perm].tolist():
                m = x if x > m else m
            assert m == st[name], (name, trial)
        for name, v in (("div_sq", dsq), ("ke_sq", ke)):
            perm = torch.randperm(v.numel(), generator=gen)
            bound = PR.SUM_BOUND * v.numel() * st[name]
            for order in (v, v.flip(0), v[perm]):
                run = 0.0
                for x in order.tolist():
                    run += x
                assert abs(run - st[name]) <= bound, (name, trial)
            assert abs(float(v[perm].sum()) - st[name]) <= bound
    # a NaN in a contribution makes that maximum NaN
    V = U.clone()
    V[2, 0, 3, 4] = float("nan")                         # on face xl (dirichlet): no interior stencil of component 2 reads it
    bad = PR.flow_stats(V, om, bcs)
    assert math.isnan(bad["rate"]) and bad["div_max"] == st["div_max"]
    V = U.clone()
    V[0, 3, 3, 4] = float("nan")
    bad = PR.flow_stats(V, om, bcs)
    assert math.isnan(bad["rate"]) and math.isnan(bad["div_max"])
    zero = PR.flow_stats(torch.zeros_like(U), om, bcs)
    assert list(zero.values()) == [0.0] * 4 and not any(math.copysign(1.0, v) < 0 for v in zero.values())


# ---- the checks in front of the device ------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """a refusal must come before context_for (and before require_gpu) is reached, in this module and in the march's"""
    def reached(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    for mod in (P, M):
        monkeypatch.setattr(mod, "context_for", reached)
        monkeypatch.setattr(mod, "require_gpu", reached)


def _calls(U, p, form, phi=None, nu=0.05):
    return [lambda: P.project(U, p, 1e-3, 1.0, None, form, phi, nu),
            lambda: P.ns_step(U, p, nu, 1e-3, form=form, phi=phi),
            lambda: P.ns_step(U, p, nu, 1e-3, None, 2, rho=1.3, form=form, phi=phi),
            lambda: P.ns_march(U, p, nu, 1e-3, 2, form=form, phi=phi),
            lambda: P.ns_march(U, p, nu, 1e-3, 2, form=form, phi=phi, cfl=0.5)]


def test_form_and_phi_checks_fire_before_a_device_is_touched(no_device):
    U = _cpu_field()
    p = _cpu_field(dim=1, name="p", mesh=U.mesh)
    for form in ("Chorin", "pressure-correction", "", None, 2):
        for call in _calls(U, p, form):
            with pytest.raises(ValueError, match="form"):
                call()
    # rotational: nu is a number
    nu_t = torch.full(tuple(U()[0].shape), 0.05, dtype=torch.float64)
    nu_f = _cpu_field(dim=1, name="nu", mesh=U.mesh)
    for nu in (nu_t, nu_f):
        for call in _calls(U, p, "rotational", None, nu):
            with pytest.raises(NotImplementedError, match="rotational"):
                call()
    for nu in (None, "thick", True):
        with pytest.raises(TypeError, match="rotational"):
            P.project(U, p, 1e-3, 1.0, None, "rotational", None, nu)
    # phi: a scalar Field of its own on U's mesh, of U's dtype and device
    for form in ("incremental", "rotational"):
        for notphi in (p(), 1.0, _cpu_field(dim=2, name="phi", mesh=U.mesh)):
            for call in _calls(U, p, form, notphi):
                with pytest.raises(TypeError, match="phi"):
                    call()
        for call in _calls(U, p, form, p):
            with pytest.raises(ValueError, match="phi is p"):
                call()
        for call in _calls(U, p, form, _cpu_field(dim=1, name="phi")):
            with pytest.raises(ValueError, match="another mesh"):
                call()
        phi32 = _cpu_field(dim=1, name="phi", mesh=U.mesh)
        phi32.set_var_tensor(torch.zeros(p().shape, dtype=torch.float32))
        for call in _calls(U, p, form, phi32):
            with pytest.raises(ValueError, match="dtype"):
                call()
        phim = _cpu_field(dim=1, name="phi", mesh=U.mesh)
        phim.set_var_tensor(torch.zeros(p().shape, dtype=torch.float64, device="meta"))
        for call in _calls(U, p, form, phim):
            with pytest.raises(ValueError, match=" on "):
                call()
        # the checks of today's arguments and of the momentum step arrive before the device on the new path too
        with pytest.raises(ValueError):
            P.ns_step(U, p, 0.05, -1e-3, form=form)
        with pytest.raises(ValueError):
            P.ns_step(U, p, 0.05, 1e-3, order=4, form=form)
        with pytest.raises(NotImplementedError):
            P.ns_step(U, p, 0.05, 1e-3, {"div": {"limiter": "upwind", "compat": True}}, form=form)
        with pytest.raises(ValueError):
            P.ns_step(U, p, 0.05, 1e-3, form=form, source=torch.zeros(3, 9, 9, dtype=torch.float64))
        with pytest.raises(ValueError):
            P.ns_step(U, p, torch.zeros(9, 8, dtype=torch.float64), 1e-3, form=form if form != "rotational" else "incremental")


def test_flow_stats_and_ns_march_checks_fire_before_a_device_is_touched(no_device):
    from pyapes_amd.geometry import Cylinder
    U = _cpu_field()
    p = _cpu_field(dim=1, name="p", mesh=U.mesh)
    # flow_stats: divergence's refusals
    for bad in (_cpu_field(n=(9, 9, 9), slab=(0, 2)), _cpu_field(geo=Cylinder[0:1, 0:1]), _cpu_field(n=(9,)),
                _cpu_field(dim=1), _cpu_field(dim=3), _cpu_field(n=(9, 9, 9), dim=2)):
        bp = _cpu_field(dim=1, name="p", mesh=bad.mesh)
        for call in (lambda: P.flow_stats(bad), lambda: P.flow_stats(bad, 1e-3), lambda: P.ns_march(bad, bp, 0.05, 1e-3, 2),
                     lambda: P.ns_march(bad, bp, 0.05, 1e-3, 2, cfl=0.4)):
            with pytest.raises(NotImplementedError):
                call()
    for notfield in (U(), None, 1.0):
        for call in (lambda: P.flow_stats(notfield), lambda: P.ns_march(notfield, p, 0.05, 1e-3, 2)):
            with pytest.raises(TypeError):
                call()
    for dt in ("fast", True):
        with pytest.raises(TypeError):
            P.flow_stats(U, dt)
    for dt in (0.0, -1e-3, float("nan")):
        with pytest.raises(ValueError):
            P.flow_stats(U, dt)
    # ns_march: ns_step's arguments, then its own
    for notp in (p(), None, _cpu_field(dim=2, name="p", mesh=U.mesh)):
        with pytest.raises(TypeError):
            P.ns_march(U, notp, 0.05, 1e-3, 2)
    for dt, rho in ((0.0, 1.0), (1e-3, -2.0), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            P.ns_march(U, p, 0.05, dt, 2, rho=rho)
    for nsteps in (2.0, "many", None, True):
        with pytest.raises(TypeError, match="nsteps"):
            P.ns_march(U, p, 0.05, 1e-3, nsteps)
    with pytest.raises(ValueError, match="nsteps"):
        P.ns_march(U, p, 0.05, 1e-3, -1)
    for cfl in ("half", True, [0.5]):
        with pytest.raises(TypeError, match="cfl"):
            P.ns_march(U, p, 0.05, 1e-3, 2, cfl=cfl)
    for cfl in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cfl"):
            P.ns_march(U, p, 0.05, 1e-3, 2, cfl=cfl)
    with pytest.raises(ValueError):
        P.ns_march(U, p, 0.05, 1e-3, 2, order=4)
    with pytest.raises(ValueError):
        P.ns_march(U, p, 0.05, 1e-3, 2, source=torch.zeros(3, 9, 9, dtype=torch.float64))
    # no step, no device: the empty march returns its empty record
    assert P.ns_march(U, p, 0.05, 1e-3, 0) == {"steps": 0, "t": 0.0, "dt": [], "itr": [], "converge": []}


def test_good_arguments_reach_the_device():
    """with every check passed the first thing each entry point asks for is the GPU (a CPU mesh: the backend's refusal)"""
    U = _cpu_field()
    p = _cpu_field(dim=1, name="p", mesh=U.mesh)
    phi = _cpu_field(dim=1, name="phi", mesh=U.mesh)
    calls = [lambda: P.flow_stats(U), lambda: P.flow_stats(U, 1e-3)]
    for form in ("incremental", "rotational"):
        calls += _calls(U, p, form) + _calls(U, p, form, phi)
    calls += [lambda: P.ns_step(U, p, torch.full((9, 9), 0.05, dtype=torch.float64), 1e-3, form="incremental"),
              lambda: P.project(U, p, 1e-3, form="incremental"), lambda: P.project(U, p, 1e-3, form="chorin", phi=phi, nu=0.1)]
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU|cuda|HIP"):
            call()


def test_the_names_are_part_of_the_package_surface():
    from pyapes_amd.hip import lib as L
    from pyapes_amd.hip.context import HipContext
    for name in ("pa_project_update", "pa_flow_stats"):
        assert name in L.SIGNATURES
    assert len(L.SIGNATURES["pa_project_update"][1]) == 9 and len(L.SIGNATURES["pa_flow_stats"][1]) == 4
    for name in ("project_update", "flow_stats"):
        assert callable(getattr(HipContext, name))
    assert P.FORMS == ("chorin", "incremental", "rotational") == PR.FORMS
    for fn, form in ((P.ns_step, "chorin"), (P.project, "chorin"), (P.ns_march, "incremental")):
        par = inspect.signature(fn).parameters
        assert par["form"].default == form and par["phi"].default is None
    assert inspect.signature(P.project).parameters["nu"].default is None
    assert inspect.signature(P.ns_march).parameters["cfl"].default is None
    assert list(inspect.signature(P.flow_stats).parameters) == ["U", "dt"]
    header = open(__file__.rsplit("/tests/", 1)[0] + "/include/pyapes_hip.h").read()
    assert "int pa_project_update(pa_ctx* ctx" in header and "int pa_flow_stats(pa_ctx* ctx" in header
