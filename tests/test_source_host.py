"""No GPU: the source term of the explicit marches, ``source=S``, on the CPU -- tests/march_ref.py (the step E_S, the stage and
the march restated operation for operation as the kernels compute them) against the oracle, what the schemes built from E_S
do, and the argument checks of pyapes_amd/solver/march.py that fire before a device is touched.

Case A (order in time), the case of tests/test_rk_host.py: 33^2 on [0, 1]^2, all faces dirichlet 0, a Gaussian pulse, u = 1,
nu = 0.05, T = 0.02, with S = 40 sin(pi x) sin(2 pi y) (it moves the end state by 0.77 in the max norm); marches of 20 / 40 /
80 steps against a 640-step order-3 march.  Max-abs error ratios under halving dt, measured on the CPU:
  order | upwind          | central
    1   | 2.014 / 2.007   | 2.012 / 2.006
    2   | 4.088 / 4.043   | 4.063 / 4.031
    3   | 8.249 / 8.136   | 8.166 / 8.096
asserted with test_rk_host.py's bounds (1.7, 2.4), (3.4, 4.8), (6.8, 9.6).  A source added between whole steps instead of in
every stage would make every order first order.

Case B (discrete fixed point): for a random phi* in [0.5, 1.5), S = -(nu lap(phi*) - adv(phi*)) formed with the step's own
rounded operations makes ``a + s`` an exact zero, so phi* is a fixed point of E_S bit for bit: 50 steps (dt = 2e-4, u = 0.7,
nu = 0.05) leave max|phi - phi*| = 0 for orders 1 and 2 and 2.2e-16 -- one ulp, from 1/3 phi + 2/3 phi -- for order 3, which
does not accumulate (every step restarts from an exact fixed point of E).

Case C (pure source): nu = 0, u = 0, 10 steps of 1e-3: phi + 10 dt S up to 1.1e-15 (orders 1, 2) / 3.1e-15 (order 3); the
S dt products are O(0.04), a few tens of ulp of the field: asserted <= 1e-13.
"""
import math

import pytest
import torch

import march_ref as R
import pyapes_oracle as O
from pyapes_amd.solver.march import euler_march, euler_step, rk_march, rk_step

N = 33
ORDER_BOUNDS = {1: (1.7, 2.4), 2: (3.4, 4.8), 3: (6.8, 9.6)}


def _case():
    mesh = O.OMesh([0.0, 0.0], [1.0, 1.0], [N, N], "double")
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(2, 0.0, "dirichlet"))
    x, y = mesh.grid
    phi = torch.exp(-((x - 0.4) ** 2 + (y - 0.5) ** 2) / 0.01).unsqueeze(0)
    O.bc_fill(phi, bcs)
    S = (40.0 * torch.sin(math.pi * x) * torch.sin(2.0 * math.pi * y)).unsqueeze(0)
    return mesh, bcs, phi, S


@pytest.mark.parametrize("limiter", ["upwind", "none"])
def test_without_a_source_the_restatement_is_the_oracle_bit_for_bit(limiter):
    mesh, bcs, phi, _ = _case()
    g = torch.Generator().manual_seed(3)
    for u in (1.0, -0.7, torch.randn(phi.shape, generator=g, dtype=phi.dtype)):
        a = R.euler_step(phi, u, 0.05, 1e-3, mesh, bcs, limiter)
        b = O.euler_step(phi, u, 0.05, 1e-3, mesh, bcs, limiter)
        assert torch.equal(a, b)
    m32 = O.OMesh([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [7, 9, 12], "single")
    b32 = O.make_bcs(m32, O.homogeneous_cfg(3, 0.25, "dirichlet"))
    p32 = torch.rand((1, 7, 9, 12), generator=g, dtype=torch.float32)
    O.bc_fill(p32, b32)
    assert torch.equal(R.euler_step(p32, 0.9, 0.05, 1e-3, m32, b32, limiter), O.euler_step(p32, 0.9, 0.05, 1e-3, m32, b32, limiter))


def test_the_source_enters_between_the_operator_and_dt():
    """E_S against the definition written out once more, and a scalar source against a tensor filled with it"""
    mesh, bcs, phi, S = _case()
    nu, dt, u = 0.05, 1e-3, 1.0
    sl = O.interior_slicer(2, bcs)
    lap, adv = R.operator_parts(phi, u, nu, mesh, bcs, "upwind")
    want = phi.clone()
    want[0][sl] = phi[0][sl] + dt * (((nu * lap[0][sl]) - adv[0][sl]) + S[0][sl])
    O.bc_fill(want, bcs)
    assert torch.equal(R.euler_step(phi, u, nu, dt, mesh, bcs, "upwind", S), want)
    assert torch.equal(R.euler_step(phi, u, nu, dt, mesh, bcs, "upwind", S[0]), want)      # one component's shape
    assert torch.equal(R.euler_step(phi, u, nu, dt, mesh, bcs, "upwind", 0.3),
                       R.euler_step(phi, u, nu, dt, mesh, bcs, "upwind", torch.full_like(phi, 0.3)))
    moved = (R.march(phi, 1.0, 0.05, 0.02 / 80, 80, mesh, bcs, "upwind", 3, S) -
             R.march(phi, 1.0, 0.05, 0.02 / 80, 80, mesh, bcs, "upwind", 3)).abs().max()
    print("the source moves the end state by", float(moved))
    assert 0.5 < float(moved) < 1.0


@pytest.mark.parametrize("limiter", ["upwind", "none"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_order_in_time_with_a_source(order, limiter):
    mesh, bcs, phi0, S = _case()
    u, nu, T = 1.0, 0.05, 0.02
    ref = R.march(phi0, u, nu, T / 640, 640, mesh, bcs, limiter, 3, S)
    err = [float((R.march(phi0, u, nu, T / n, n, mesh, bcs, limiter, order, S) - ref).abs().max()) for n in (20, 40, 80)]
    ratios = (err[0] / err[1], err[1] / err[2])
    print(f"order {order} {limiter}: errors {err}, ratios {ratios}")
    lo, hi = ORDER_BOUNDS[order]
    for r in ratios:
        assert lo < r < hi, (order, limiter, err, ratios)


@pytest.mark.parametrize("limiter", ["upwind", "none", "quick"])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_discrete_fixed_point(order, limiter):
    mesh, bcs, _, _ = _case()
    g = torch.Generator().manual_seed(11)
    star = torch.rand((1, N, N), generator=g, dtype=torch.float64) + 0.5
    O.bc_fill(star, bcs)
    u, nu, dt = 0.7, 0.05, 2e-4
    S = R.fixed_point_source(star, u, nu, mesh, bcs, limiter)
    end = R.march(star, u, nu, dt, 50, mesh, bcs, limiter, order, S)
    dev = float((end - star).abs().max())
    print(f"order {order} {limiter}: max|phi - phi*| = {dev:.3e}")
    if order < 3:
        assert torch.equal(end, star)
    else:
        ulp = float(torch.finfo(torch.float64).eps) * float(star.abs().max())
        assert dev <= 4 * ulp, (dev, ulp)


@pytest.mark.parametrize("order", [1, 2, 3])
def test_pure_source(order):
    mesh, bcs, phi, S = _case()
    dt = 1e-3
    end = R.march(phi, 0.0, 0.0, dt, 10, mesh, bcs, "upwind", order, S)
    sl = O.interior_slicer(2, bcs)
    want = phi[0][sl] + 10 * dt * S[0][sl]
    dev = float((end[0][sl] - want).abs().max())
    print(f"order {order}: deviation from phi + 10 dt S = {dev:.3e}")
    assert dev <= 1e-13


# ---- the checks in front of the device -------------------------------------------------------------------------------
def _cpu_field(n=(9, 9), dim=1, slab=None, geo=None):
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    box = geo if geo is not None else (Box[0:1, 0:1] if len(n) == 2 else Box[0:1, 0:1, 0:1])
    kw = {"slab": slab} if slab else {}
    mesh = Mesh(box, None, list(n), "cpu", "double", **kw)     # a CPU mesh: anything past the argument checks raises RuntimeError
    cfg = mixed_bcs([0.0] * (2 * len(n)), ["dirichlet"] * (2 * len(n)))
    if geo is not None:   # an axisymmetric mesh names its faces rl, ru, zl, zu
        cfg = [dict(c, bc_face=f) for c, f in zip(cfg, O.FACES_RZ)]
    return Field("phi", dim, mesh, {"domain": cfg, "obstacle": None})


def _calls(phi, **kw):
    """the four public entry points (rk at orders 1 .. 3) as thunks"""
    out = [lambda: euler_step(phi, 1.0, 0.05, 1e-3, **kw), lambda: euler_march(phi, 1.0, 0.05, 1e-3, 2, **kw)]
    for order in (1, 2, 3):
        out.append(lambda order=order: rk_step(phi, 1.0, 0.05, 1e-3, order=order, **kw))
        out.append(lambda order=order: rk_march(phi, 1.0, 0.05, 1e-3, 2, order=order, **kw))
    return out


def test_source_is_keyword_only():
    phi = _cpu_field()
    with pytest.raises(TypeError):
        euler_step(phi, 1.0, 0.05, 1e-3, None, 1.0)
    with pytest.raises(TypeError):
        rk_march(phi, 1.0, 0.05, 1e-3, 2, None, 3, 1.0)


def test_source_argument_checks_fire_before_a_device_is_touched():
    from pyapes_amd.geometry import Cylinder
    phi = _cpu_field()
    shape = phi().shape
    bad_values = [
        torch.zeros(1, 9, 8, dtype=torch.float64),          # wrong shape
        torch.zeros(9, 8, dtype=torch.float64),
        torch.zeros(2, 9, 9, dtype=torch.float64),
        torch.zeros(shape, dtype=torch.float32),            # wrong dtype
        phi(),                                              # phi's own tensor
        phi()[0],                                           # a view on phi's storage
    ]
    if torch.cuda.is_available():
        bad_values.append(torch.zeros(shape, dtype=torch.float64, device="cuda"))   # wrong device
    for bad in bad_values:
        for call in _calls(phi, source=bad):
            with pytest.raises(ValueError):
                call()
    vec = _cpu_field(dim=2)
    other = _cpu_field()
    for call in _calls(phi, source=vec):                    # a vector Field
        with pytest.raises(NotImplementedError):
            call()
    for call in _calls(phi, source=other):                  # a scalar Field, but on another mesh
        with pytest.raises(ValueError):
            call()
    for call in _calls(phi, source="heater"):
        with pytest.raises(TypeError):
            call()
    slab = _cpu_field(n=(9, 9, 9), slab=(0, 2))
    rz = _cpu_field(geo=Cylinder[0:1, 0:1])
    for f in (slab, rz):
        for src in (1.0, torch.zeros(f().shape, dtype=torch.float64)):
            for call in _calls(f, source=src):
                with pytest.raises(NotImplementedError):
                    call()


def test_a_good_source_and_none_get_past_the_checks():
    """past the argument checks a CPU mesh fails where it does today: the march itself needs the GPU (RuntimeError, not one of
    the checks' own NotImplementedError)"""
    phi = _cpu_field()
    from pyapes_amd.variables.bcs import mixed_bcs
    same_mesh = type(phi)("s", 1, phi.mesh, {"domain": mixed_bcs([0.0] * 4, ["dirichlet"] * 4), "obstacle": None})
    good = [None, 1.5, 2, torch.ones(phi().shape, dtype=torch.float64), torch.ones(9, 9, dtype=torch.float64),
            torch.ones(9, 18, dtype=torch.float64)[:, ::2], same_mesh]
    for src in good:
        for call in _calls(phi, source=src):
            with pytest.raises(RuntimeError) as ei:
                call()
            assert ei.type is RuntimeError, (src, ei.value)
    for call in _calls(phi):                                # the argument left out
        with pytest.raises(RuntimeError) as ei:
            call()
        assert ei.type is RuntimeError
