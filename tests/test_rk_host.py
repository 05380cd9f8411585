"""No GPU: the SSP Runge-Kutta stage table of pyapes_amd/solver/march.py and what the schemes built from it do, on the
CPU, composed by tests/march_ref.py from the oracle's own Euler step (oracle.euler_step, the function the GPU Euler step is
pinned against).

A stage of a step is  c0 * phi0 + c1 * E(phi_s)  (Shu-Osher form); the plain first stage phi1 = E(phi0) is implied.
  order 2:  phi' = 1/2 phi0 + 1/2 E(phi1)
  order 3:  phi2 = 3/4 phi0 + 1/4 E(phi1);  phi' = 1/3 phi0 + 2/3 E(phi2)

Case A (order in time): 33^2 on [0, 1]^2, all faces dirichlet 0, a Gaussian pulse, u = 1, nu = 0.05, T = 0.02; marches of
20 / 40 / 80 steps against a 640-step order-3 march.  Max-abs error ratios under halving dt, measured on the CPU:
  order | upwind 1st  2nd | central 1st  2nd
    1   |  2.02   2.01    |  2.02   2.01
    2   |  4.10   4.05    |  4.07   4.04
    3   |  8.25   8.14    |  8.19   8.10
asserted against theory's 2 / 4 / 8 with the margin those show: (1.7, 2.4), (3.4, 4.8), (6.8, 9.6).  Dirichlet faces on
purpose: with the reference's periodic fill (error floor ~1e-7) the order-3 ratio decays to 2.3-3.9 at these step sizes.

Case B (stability): same mesh and pulse, nu = 0, central Div, dt = CFL dx / u.  max|phi| at the end, measured:
  CFL 1.0, 8 steps: Euler 4.66, order 2 1.37, order 3 0.886;   CFL 1.5, 5 steps: 5.21 / 3.17 / 0.924.
"""
from fractions import Fraction

import pytest
import torch

import march_ref
import pyapes_oracle as O
from pyapes_amd.solver.march import SSP_STAGES, rk_march, rk_step

N = 33
ORDER_BOUNDS = {1: (1.7, 2.4), 2: (3.4, 4.8), 3: (6.8, 9.6)}


def _case():
    mesh = O.OMesh([0.0, 0.0], [1.0, 1.0], [N, N], "double")
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(2, 0.0, "dirichlet"))
    x, y = mesh.grid
    phi = torch.exp(-((x - 0.4) ** 2 + (y - 0.5) ** 2) / 0.01).unsqueeze(0)
    O.bc_fill(phi, bcs)
    return mesh, bcs, phi


def test_stage_table_is_convex_and_sums_to_one():
    for order, stages in SSP_STAGES.items():
        for c0, c1 in stages:
            f0, f1 = Fraction(c0).limit_denominator(12), Fraction(c1).limit_denominator(12)
            assert f0 + f1 == 1, (order, f0, f1)
            assert c0 > 0 and c1 > 0
            assert abs(float(f0) - c0) < 1e-15 and abs(float(f1) - c1) < 1e-15   # the table holds those fractions


def test_number_of_fused_stages_per_order():
    assert sorted(SSP_STAGES) == [1, 2, 3]
    assert [len(SSP_STAGES[o]) for o in (1, 2, 3)] == [0, 1, 2]


def test_bad_order_raises_before_a_device_is_touched():
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    mesh = Mesh(Box[0:1, 0:1], None, [9, 9], "cpu", "double")    # a CPU mesh: anything past the argument check raises RuntimeError
    phi = Field("phi", 1, mesh, {"domain": mixed_bcs([0.0] * 4, ["dirichlet"] * 4), "obstacle": None})
    for bad in (4, 0, -1, 2.5, None):
        with pytest.raises(ValueError):
            rk_march(phi, 1.0, 0.05, 1e-3, 2, order=bad)
        with pytest.raises(ValueError):
            rk_step(phi, 1.0, 0.05, 1e-3, order=bad)


@pytest.mark.parametrize("limiter", ["upwind", "none"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_order_in_time(order, limiter):
    mesh, bcs, phi0 = _case()
    u, nu, T = 1.0, 0.05, 0.02
    ref = march_ref.march(phi0, u, nu, T / 640, 640, mesh, bcs, limiter, 3, step=O.euler_step)
    err = [float((march_ref.march(phi0, u, nu, T / n, n, mesh, bcs, limiter, order, step=O.euler_step) - ref).abs().max())
           for n in (20, 40, 80)]
    ratios = (err[0] / err[1], err[1] / err[2])
    print(f"order {order} {limiter}: errors {err}, ratios {ratios}")
    lo, hi = ORDER_BOUNDS[order]
    for r in ratios:
        assert lo < r < hi, (order, limiter, err, ratios)


def test_order_three_marches_central_advection_that_euler_cannot():
    mesh, bcs, phi0 = _case()
    top = float(phi0.abs().max())
    dx = mesh.dx_list[0]
    ends = {}
    for cfl, steps in ((1.0, 8), (1.5, 5)):
        for order in (1, 2, 3):
            ends[cfl, order] = float(march_ref.march(phi0, 1.0, 0.0, cfl * dx / 1.0, steps, mesh, bcs, "none", order, step=O.euler_step).abs().max())
    print("max|phi| at the end:", ends)
    assert ends[1.0, 3] <= top and ends[1.5, 3] <= top, ends
    assert ends[1.0, 1] >= 2 * top, ends
