"""No GPU: self-advection, div(phi, phi), marched by the SSP Runge-Kutta schemes of pyapes_amd/solver/march.py -- what the
schemes do when every stage is advected by ITS OWN input, composed on the CPU from the oracle's Euler step with the field
handed in as its own speed, O.euler_step(phi, phi, ...); and the host-side rule that decides when a march is a
self-advected one.

A stage is  B(c0 phi0 + c1 E_self(phi_s)),  E_self(p) = B(p + dt (nu lap(p) - Div(u = p, p))):  the speed is phi_s, never phi0.

Case A (order in time): the pulse case of tests/test_rk_host.py (33^2 on [0, 1]^2, dirichlet 0, nu = 0.05, T = 0.02), marches
of 20 / 40 / 80 steps against a 640-step order-3 self march.  Max-abs error ratios under halving dt, measured on the CPU:
  order | upwind 1st  2nd | central 1st  2nd
    1   |  2.02   2.01    |  2.02   2.01
    2   |  4.11   4.05    |  4.12   4.06
    3   |  8.31   8.16    |  8.16   8.09
against test_rk_host.py's bounds (1.7, 2.4), (3.4, 4.8), (6.8, 9.6).  The same march with the stages advected by the step's
STARTING state (a stale speed) is first order whatever the stage table: ratios 1.93-2.02 at orders 2 and 3 -- the
counter-example that shows the bounds tell the two apart.

Case B (Burgers' equation u_t + u u_x = nu u_xx, 1-D on [0, 2 pi], nu = 0.5, T = 0.1, the exact solution of the reference's
pyapes/testing/burgers.py restated below; dirichlet values fixed at the t = 0 end values; order 3, 200 (N // 100)^2 steps;
max error over the middle half [N // 4, 3 N // 4)):
  central Div marches phi_t + (phi^2)_x = nu phi_xx, so phi = u / 2 is marched and 2 phi compared:
      N = 101: 1.845e-2, N = 201: 4.634e-3  -- asserted <= 2.2e-2 and ratio >= 3.5 (a 20 % margin on these)
  upwind Div is u (phi - phi[-1]) / dx for u > 0, marched from the exact solution itself:
      2.057e-1 -> 1.106e-1, first order in space -- the ratio asserted inside (1.6, 2.2)
"""
import math

import pytest
import torch

import march_ref
import pyapes_oracle as O
from pyapes_amd.solver.march import advects_itself, euler_march, rk_march, rk_step

ORDER_BOUNDS = {1: (1.7, 2.4), 2: (3.4, 4.8), 3: (6.8, 9.6)}
BURGERS_NU, BURGERS_T = 0.5, 0.1


def oracle_self_march(phi, nu, dt, nsteps, mesh, bcs, limiter, order):
    """every stage B(c0 phi0 + c1 E(phi_s)) with the oracle's E advected by phi_s itself"""
    return march_ref.march(phi, None, nu, dt, nsteps, mesh, bcs, limiter, order, self_adv=True, step=O.euler_step)


def stale_self_march(phi, nu, dt, nsteps, mesh, bcs, limiter, order):
    """the wrong scheme: the stages advected by the step's starting state phi0 instead of their own input"""
    for _ in range(nsteps):
        phi0 = phi
        phi = O.euler_step(phi0, phi0, nu, dt, mesh, bcs, limiter)
        for c0, c1 in march_ref.SSP_STAGES[order]:
            phi = march_ref.rk_stage(phi, phi0, c0, c1, phi0, nu, dt, mesh, bcs, limiter, step=O.euler_step)
    return phi


def pulse_case():
    mesh = O.OMesh([0.0, 0.0], [1.0, 1.0], [33, 33], "double")
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(2, 0.0, "dirichlet"))
    x, y = mesh.grid
    phi = torch.exp(-((x - 0.4) ** 2 + (y - 0.5) ** 2) / 0.01).unsqueeze(0)
    O.bc_fill(phi, bcs)
    return mesh, bcs, phi


def order_ratios(march):
    """march(nsteps, order) -> field; error ratios of 20 / 40 / 80 steps against the 640-step order-3 march"""
    ref = march(640, 3, False)
    out = {}
    for order in (1, 2, 3):
        for stale in (False, True):
            if stale and order == 1:
                continue
            err = [float((march(n, order, stale) - ref).abs().max()) for n in (20, 40, 80)]
            out[order, stale] = (err[0] / err[1], err[1] / err[2])
    return out


@pytest.mark.parametrize("limiter", ["upwind", "none"])
def test_order_in_time_of_the_self_advected_march(limiter):
    mesh, bcs, phi0 = pulse_case()
    nu, T = 0.05, 0.02
    ratios = order_ratios(lambda n, order, stale: (stale_self_march if stale else oracle_self_march)(phi0, nu, T / n, n, mesh, bcs, limiter, order))
    print(limiter, ratios)
    for order in (1, 2, 3):
        lo, hi = ORDER_BOUNDS[order]
        for r in ratios[order, False]:
            assert lo < r < hi, (order, limiter, ratios)
    # a stage advected by the step's starting state: first order, outside the bounds of its nominal order
    for order in (2, 3):
        lo, _ = ORDER_BOUNDS[order]
        for r in ratios[order, True]:
            assert 1.7 < r < 2.4 and r < lo, (order, limiter, ratios)


def burgers_exact(x, nu, t):
    """u(x, t) = -2 nu phi_x / phi + 4,  phi = exp(-(x - 4t)^2 / (4 nu (t + 1))) + exp(-(x - 4t - 2 pi)^2 / (4 nu (t + 1)))"""
    a, b = x - 4 * t, x - 4 * t - 2 * math.pi
    d = 4 * nu * (t + 1)
    ea, eb = torch.exp(-a * a / d), torch.exp(-b * b / d)
    dphi = -(2 * a / d) * ea - (2 * b / d) * eb
    return -2 * nu * dphi / (ea + eb) + 4


def burgers_error(n, limiter, march):
    """march(start (1, n) tensor, end values (lo, hi), dt, steps) -> (1, n) tensor;  the error of Case B"""
    x = torch.linspace(0.0, 2 * math.pi, n, dtype=torch.float64)
    scale = 2.0 if limiter == "none" else 1.0          # central Div marches u / 2
    start = (burgers_exact(x, BURGERS_NU, 0.0) / scale).unsqueeze(0)
    steps = 200 * (n // 100) ** 2
    end = march(start, (float(start[0, 0]), float(start[0, -1])), BURGERS_T / steps, steps)
    exact = burgers_exact(x, BURGERS_NU, BURGERS_T)
    mid = slice(n // 4, 3 * n // 4)
    return float((scale * end.to("cpu", torch.float64)[0] - exact)[mid].abs().max())


def _oracle_burgers(limiter):
    def march(start, ends, dt, steps):
        n = start.shape[1]
        mesh = O.OMesh([0.0], [2 * math.pi], [n], "double")
        bcs = O.make_bcs(mesh, O.mixed_cfg(list(ends), ["dirichlet", "dirichlet"]))
        phi = O.bc_fill(start.clone(), bcs)
        return oracle_self_march(phi, BURGERS_NU, dt, steps, mesh, bcs, limiter, 3)
    return march


def test_burgers_central():
    e1, e2 = (burgers_error(n, "none", _oracle_burgers("none")) for n in (101, 201))
    print(f"central: {e1:.4e} {e2:.4e} ratio {e1 / e2:.3f}")
    assert e1 <= 2.2e-2 and e1 / e2 >= 3.5, (e1, e2)


def test_burgers_upwind():
    e1, e2 = (burgers_error(n, "upwind", _oracle_burgers("upwind")) for n in (101, 201))
    print(f"upwind: {e1:.4e} {e2:.4e} ratio {e1 / e2:.3f}")
    assert 1.6 < e1 / e2 < 2.2, (e1, e2)


# ---- the host-side rule and the checks in front of the device --------------------------------------------------------
def _cpu_field(n=(9, 9), dim=1, slab=None):
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    box = Box[0:1, 0:1] if len(n) == 2 else Box[0:1, 0:1, 0:1]
    kw = {"slab": slab} if slab else {}
    mesh = Mesh(box, None, list(n), "cpu", "double", **kw)     # a CPU mesh: anything past the argument checks raises RuntimeError
    return Field("phi", dim, mesh, {"domain": mixed_bcs([0.0] * (2 * len(n)), ["dirichlet"] * (2 * len(n))), "obstacle": None})


def test_self_detection_rule():
    phi, other = _cpu_field(), _cpu_field()
    phi.set_var_tensor(torch.rand_like(phi()))
    assert advects_itself(phi, phi)                          # identity
    assert advects_itself(phi, phi())                        # the field's own tensor
    assert advects_itself(phi, phi().view(phi().shape))      # another tensor object on the same storage, same shape
    other.set_var_tensor(phi())
    assert advects_itself(phi, other)                        # a Field on phi's storage
    assert not advects_itself(phi, phi().clone())            # a clone is a frozen speed
    other.set_var_tensor(phi().clone())
    assert not advects_itself(phi, other)
    assert not advects_itself(phi, 1.0) and not advects_itself(phi, 0)
    assert not advects_itself(phi, phi()[0])                 # same pointer, another shape
    big = torch.zeros(2, *phi().shape[1:], dtype=phi().dtype)
    phi.set_var_tensor(big[:1])
    assert not advects_itself(phi, big[1:]) and advects_itself(phi, big[:1])


def test_self_advection_argument_checks_fire_before_a_device_is_touched():
    vec = _cpu_field(dim=2)
    slab = _cpu_field(n=(9, 9, 9), slab=(0, 2))
    for f in (vec, slab):
        with pytest.raises(NotImplementedError):
            euler_march(f, f, 0.05, 1e-3, 2)
        for order in (1, 2, 3):
            with pytest.raises(NotImplementedError):
                rk_march(f, f, 0.05, 1e-3, 2, order=order)
            with pytest.raises(NotImplementedError):
                rk_step(f, f, 0.05, 1e-3, order=order)
    with pytest.raises(NotImplementedError):
        euler_march(slab, slab(), 0.05, 1e-3, 2)             # the field's own tensor is self-advection as well
    phi = _cpu_field()
    for bad in (0, 4, None):
        with pytest.raises(ValueError):
            rk_march(phi, phi, 0.05, 1e-3, 2, order=bad)
    with pytest.raises(RuntimeError):                        # past the checks: the march itself needs the GPU
        rk_march(phi, phi, 0.05, 1e-3, 2, order=3)
    with pytest.raises(RuntimeError):
        euler_march(phi, phi, 0.05, 1e-3, 2)
