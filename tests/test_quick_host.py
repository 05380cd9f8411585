"""No GPU: the QUICK advection scheme (Div limiter "quick"), restated on the CPU in tests/march_ref.py, and the host-side
checks in front of the device.  Figures are what the restatement gives on the CPU (float64); bounds carry about 20 % margin.

1. Quadratic 1 + 2x - y + 3z + x^2 - 2y^2 + z^2/2 on 9 x 11 x 13, u = 1.3 and -0.7: exact at every interior node (the central
   fallback next to a face is exact for quadratics too).  Measured max error 3.6e-14 / 1.7e-14, asserted <= 1e-12.
2. Cubic x^3 on 9 nodes of [0, 1], u = 1: the error is dx^2 / 4 = 0.00390625 at i >= 2 (QUICK: dx^2/4 x'''/6 ... x''' = 6) and
   dx^2 = 0.015625 at i = 1 (central: dx^2/6 x'''), each to 1e-12 (measured: 3e-16 off) -- this pins where the fallback sits.
3. Mirror: 201 nodes on [0, 2], dirichlet 0, nu = 0, 50 order-3 steps at CFL 0.4: a Gaussian with u = 1 equals bit for bit the
   flipped result of the flipped Gaussian with u = -1.
4. Advected Gaussian exp(-(x - 0.6)^2 / 0.01) on [0, 2], u = 1, nu = 0, T = 0.4, order 3, CFL 0.4, N = 101 / 201 / 401.
   Max error   QUICK 3.337e-2, 7.259e-3, 1.680e-3 (ratios 4.60, 4.32)
               central 1.032e-1, 2.638e-2, 6.536e-3;   upwind 3.80e-1, 2.55e-1, 1.55e-1.
   Asserted: e(101) <= 4.0e-2, both ratios >= 3.5, QUICK <= 0.4 x central at each N, QUICK <= 0.1 x upwind at N = 201.
5. Stability: 129 nodes on [0, 1], torch.rand seed 0, dirichlet 0, u = 1, nu = 0, 600 steps.  Forward Euler at CFL 0.5 ends with
   max 1.8e19 (asserted > 1e6); order 3 at CFL 1.0 ends at 3e-82 (asserted <= 1.0: the inflow flushes the field).
6. Order in time: the pulse case of tests/test_rk_host.py (33^2, nu = 0.05, T = 0.02, 20 / 40 / 80 steps against 640).  Ratios
   u = 1: 2.02/2.01, 4.08/4.04, 8.18/8.10; self-advected: 2.02/2.01, 4.11/4.05, 8.28/8.15 -- inside ORDER_BOUNDS.
7. Burgers (burgers_error of tests/test_self_march_host.py, scale 1, self-advected, order 3): 7.241e-3 (N = 101), 1.812e-3
   (N = 201), ratio 4.00.  Asserted e1 <= 8.7e-3, ratio >= 3.4, e1 <= 0.1 x upwind's 2.057e-1.
8. Host checks, each on a CPU mesh before any device call.
"""
import math

import pytest
import torch

import march_ref as Q
import pyapes_oracle as O
from test_rk_host import ORDER_BOUNDS, _case as pulse_case
from test_self_march_host import BURGERS_NU, burgers_error

from pyapes_amd.hip import lib as L
from pyapes_amd.solver.fdc import FDC, div_kind
from pyapes_amd.solver.march import SSP_STAGES, euler_march, euler_step, rk_march, rk_step

QUICK = {"div": {"limiter": "quick"}}


def test_stage_table_is_the_library_s():
    assert Q.SSP_STAGES == SSP_STAGES


@pytest.mark.parametrize("u", [1.3, -0.7])
def test_quadratics_are_exact(u):
    mesh = O.OMesh([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [9, 11, 13], "double")
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(3, 0.0, "dirichlet"))
    x, y, z = mesh.grid
    phi = (1 + 2 * x - y + 3 * z + x * x - 2 * y * y + 0.5 * z * z).unsqueeze(0)
    exact = u * ((2 + 2 * x) + (-1 - 4 * y) + (3 + z))
    S = (slice(1, -1),) * 3
    err = float((Q.div_quick(u, phi, mesh, bcs)[0] - exact)[S].abs().max())
    print(f"quadratic u={u}: max error {err:.3e}")
    assert err <= 1e-12


def test_cubic_error_pins_the_fallback():
    mesh = O.OMesh([0.0], [1.0], [9], "double")
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(1, 0.0, "dirichlet"))
    x = mesh.grid[0]
    dx = mesh.dx_list[0]
    err = (Q.div_quick(1.0, (x ** 3).unsqueeze(0), mesh, bcs)[0] - 3 * x * x).abs()
    print("cubic:", err.tolist())
    assert abs(dx * dx / 4 - 0.00390625) < 1e-15
    for i in range(2, 8):
        assert abs(float(err[i]) - dx * dx / 4) <= 1e-12, (i, float(err[i]))
    assert abs(float(err[1]) - dx * dx) <= 1e-12, float(err[1])


def _line(n, hi=2.0):
    mesh = O.OMesh([0.0], [hi], [n], "double")
    return mesh, O.make_bcs(mesh, O.homogeneous_cfg(1, 0.0, "dirichlet"))


def _gauss(mesh, bcs, centre):
    x = mesh.grid[0]
    return O.bc_fill(torch.exp(-((x - centre) ** 2) / 0.01).unsqueeze(0), bcs)


def test_mirror_symmetry_bit_for_bit():
    mesh, bcs = _line(201)
    g = _gauss(mesh, bcs, 0.6)
    dt = 0.4 * mesh.dx_list[0]
    a = Q.march(g, 1.0, 0.0, dt, 50, mesh, bcs, "quick", 3)
    b = Q.march(torch.flip(g, [1]).contiguous(), -1.0, 0.0, dt, 50, mesh, bcs, "quick", 3)
    assert torch.equal(a, torch.flip(b, [1]))
    assert float((a - g).abs().max()) > 0.1     # it moved


def advected_gaussian_errors(march):
    """march(mesh, bcs, start, dt, nsteps, limiter) -> end;  {limiter: [max error at N = 101, 201, 401]}"""
    out = {}
    for limiter in ("quick", "none", "upwind"):
        errs = []
        for n in (101, 201, 401):
            mesh, bcs = _line(n)
            nsteps = (n - 1) // 2                     # T = 0.4 at CFL 0.4, u = 1: dt = 0.4 dx, 1 / dx steps
            dt = 0.4 / nsteps
            end = march(mesh, bcs, _gauss(mesh, bcs, 0.6), dt, nsteps, limiter)
            exact = torch.exp(-((mesh.grid[0] - 1.0) ** 2) / 0.01)
            errs.append(float((end.to("cpu", torch.float64)[0] - exact).abs().max()))
        out[limiter] = errs
    return out


def check_advected_gaussian(e):
    q, c, w = e["quick"], e["none"], e["upwind"]
    print("advected Gaussian, max error:", e, "ratios", q[0] / q[1], q[1] / q[2])
    assert q[0] <= 4.0e-2, q
    assert q[0] / q[1] >= 3.5 and q[1] / q[2] >= 3.5, q
    for i in range(3):
        assert q[i] <= 0.4 * c[i], (i, q, c)
    assert q[1] <= 0.1 * w[1], (q, w)


def test_advected_gaussian():
    def march(mesh, bcs, start, dt, nsteps, limiter):
        if limiter == "quick":
            return Q.march(start, 1.0, 0.0, dt, nsteps, mesh, bcs, "quick", 3)
        return Q.march(start, 1.0, 0.0, dt, nsteps, mesh, bcs, limiter, 3, step=O.euler_step)
    check_advected_gaussian(advected_gaussian_errors(march))


def stability_start():
    torch.manual_seed(0)
    return torch.rand(129, dtype=torch.float64).unsqueeze(0)


def test_stability_needs_the_order_three_march():
    mesh, bcs = _line(129, 1.0)
    start = O.bc_fill(stability_start(), bcs)
    dx = mesh.dx_list[0]
    euler = float(Q.march(start, 1.0, 0.0, 0.5 * dx, 600, mesh, bcs, "quick", 1).abs().max())
    rk3 = float(Q.march(start, 1.0, 0.0, 1.0 * dx, 600, mesh, bcs, "quick", 3).abs().max())
    print(f"stability: Euler CFL 0.5 -> {euler:.3e}, order 3 CFL 1.0 -> {rk3:.3e}")
    assert euler > 1e6
    assert rk3 <= 1.0


@pytest.mark.parametrize("self_adv", [False, True], ids=["u=1", "self"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_order_in_time(order, self_adv):
    mesh, bcs, phi0 = pulse_case()
    nu, T = 0.05, 0.02
    ref = Q.march(phi0, 1.0, nu, T / 640, 640, mesh, bcs, "quick", 3, self_adv=self_adv)
    err = [float((Q.march(phi0, 1.0, nu, T / n, n, mesh, bcs, "quick", order, self_adv=self_adv) - ref).abs().max()) for n in (20, 40, 80)]
    ratios = (err[0] / err[1], err[1] / err[2])
    print(f"order {order} self {self_adv}: errors {err}, ratios {ratios}")
    lo, hi = ORDER_BOUNDS[order]
    for r in ratios:
        assert lo < r < hi, (order, self_adv, err, ratios)


def check_burgers(e1, e2):
    print(f"Burgers, quick: {e1:.4e} {e2:.4e} ratio {e1 / e2:.3f}")
    assert e1 <= 8.7e-3, e1
    assert e1 / e2 >= 3.4, (e1, e2)
    assert e1 <= 0.1 * 2.057e-1, e1


def test_burgers_second_order():
    def march(start, ends, dt, steps):
        n = start.shape[1]
        mesh = O.OMesh([0.0], [2 * math.pi], [n], "double")
        bcs = O.make_bcs(mesh, O.mixed_cfg(list(ends), ["dirichlet", "dirichlet"]))
        return Q.march(O.bc_fill(start.clone(), bcs), None, BURGERS_NU, dt, steps, mesh, bcs, "quick", 3, self_adv=True)
    check_burgers(*(burgers_error(n, "quick", march) for n in (101, 201)))


# ---- the checks in front of the device ------------------------------------------------------------------------------
def _cpu_field(n=(9, 9), dim=1, slab=None, cyl=False):
    from pyapes_amd.geometry import Box, Cylinder
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import CylinderBoundary, mixed_bcs
    if cyl:
        mesh = Mesh(Cylinder[0:1, 0:1], None, list(n), "cpu", "double")
        d = {"bc_type": "dirichlet", "bc_val": 0.0}
        return Field("phi", dim, mesh, {"domain": CylinderBoundary(rl={"bc_type": "neumann", "bc_val": 0.0}, ru=d, zl=d, zu=d)(),
                                        "obstacle": None})
    box = Box[0:1, 0:1] if len(n) == 2 else Box[0:1, 0:1, 0:1]
    kw = {"slab": slab} if slab else {}
    mesh = Mesh(box, None, list(n), "cpu", "double", **kw)     # a CPU mesh: anything past the argument checks raises RuntimeError
    return Field("phi", dim, mesh, {"domain": mixed_bcs([0.0] * (2 * len(n)), ["dirichlet"] * (2 * len(n))), "obstacle": None})


def _needs_gpu(call):
    """the usual RuntimeError of a CPU mesh -- and not its subclass NotImplementedError, which is what a refusal raises"""
    with pytest.raises(RuntimeError) as e:
        call()
    assert not isinstance(e.value, NotImplementedError), e.value


def test_div_kind_knows_quick():
    assert L.OP_DIV_QUICK == 5
    assert div_kind("quick", False) == L.OP_DIV_QUICK
    with pytest.raises(ValueError):
        div_kind("quick", True)


def test_quick_is_explicit_only():
    from pyapes_amd.solver.fdm import FDM
    from pyapes_amd.solver.ops import Solver
    phi = _cpu_field()
    fdm = FDM(QUICK)
    solver = Solver({"fdm": {"method": "bicgstab", "tol": 1e-6, "max_it": 10, "report": False}})
    with pytest.raises(NotImplementedError, match="explicit-only"):
        solver.set_eq(fdm.div(1.0, phi) - fdm.laplacian(0.1, phi) == 0.0)
    with pytest.raises(NotImplementedError, match="explicit-only"):
        FDC(QUICK).div.adjust_rhs(1.0, phi, QUICK)


def test_quick_argument_checks_fire_before_a_device_is_touched():
    slab = _cpu_field(n=(9, 9, 9), slab=(0, 2))
    cyl = _cpu_field(cyl=True)
    vec = _cpu_field(dim=2)
    for f in (slab, cyl):
        with pytest.raises(NotImplementedError):
            euler_step(f, 1.0, 0.05, 1e-3, QUICK)
        with pytest.raises(NotImplementedError):
            euler_march(f, 1.0, 0.05, 1e-3, 2, QUICK)
        with pytest.raises(NotImplementedError):
            rk_step(f, 1.0, 0.05, 1e-3, QUICK, order=3)
        with pytest.raises(NotImplementedError):
            rk_march(f, 1.0, 0.05, 1e-3, 2, QUICK, order=2)
        with pytest.raises(NotImplementedError):
            FDC(QUICK).div(1.0, f)
    with pytest.raises(NotImplementedError):
        rk_march(vec, 1.0, 0.05, 1e-3, 2, QUICK)
    with pytest.raises(NotImplementedError):
        euler_march(vec, 1.0, 0.05, 1e-3, 2, QUICK)
    with pytest.raises(NotImplementedError):
        FDC(QUICK).div(1.0, vec)                                       # a vector field
    phi = _cpu_field()
    with pytest.raises(NotImplementedError):
        FDC({"div": {"limiter": "quick", "edge": True}}).div(1.0, phi)   # edge=True
    with pytest.raises(ValueError):
        rk_march(phi, 1.0, 0.05, 1e-3, 2, {"div": {"limiter": "quick", "compat": True}})
    # past the checks: the operator and the marches need the GPU
    _needs_gpu(lambda: FDC(QUICK).div(1.0, phi))
    _needs_gpu(lambda: rk_march(phi, 1.0, 0.05, 1e-3, 2, QUICK, order=3))
    _needs_gpu(lambda: rk_march(phi, phi, 0.05, 1e-3, 2, QUICK, order=3))
    _needs_gpu(lambda: rk_step(phi, 1.0, 0.05, 1e-3, QUICK, order=2))
    _needs_gpu(lambda: euler_march(phi, 1.0, 0.05, 1e-3, 2, QUICK))
    _needs_gpu(lambda: euler_step(phi, 1.0, 0.05, 1e-3, QUICK))
