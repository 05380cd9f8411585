"""No GPU: the diffusivity field of the explicit marches -- tests/march_ref.py (the term div(nu grad phi), nu per node, and the step
that carries it, restated operation for operation as the kernels compute them) against the oracle and against what a
conservative diffusion operator must do, and the argument checks of pyapes_amd/solver/march.py that fire before a device is
touched.

1. nu == 1 reproduces the oracle's Laplacian: integer-valued phi in [-8, 8], dx = 0.25 on a 5 x 9 x 17 all-dirichlet mesh; every
   operation is exact in fp32 and fp64 (w = 0.5 * 16, nup = num = 2, integer differences), so the term equals
   apply_laplacian(laplacian_tables) bit for bit on the interior set.
2. Discrete steady state: 1-D, 17 nodes, dirichlet 0 / 1, nu = 1 at nodes below 8 and 4 from node 8 on; phi_i the normalised
   cumulative sum of 1 / nu_{i+1/2}, formed in fp64 and rounded.  The two face fluxes of a node are analytically equal, so the
   Euler step's increment on the interior set is rounding: two rounded products and one difference of rounded operands, at most
   16 eps max|nup fp| w dt.
3. Conservation: 12 x 11 x 16, dirichlet 0, phi nonzero only in [3:9, 3:8, 4:12], random nu >= 0.1, u = 0.  The sum of the step's
   increments telescopes face by face; what is left is rounding, |sum(v - phi)| <= 64 eps sum|dt w_a nup fp| over faces and axes.
4. Every refusal of the Python layer, each made without a GPU.
"""
import pytest
import torch

import march_ref as R
import pyapes_oracle as O
from pyapes_amd.solver.march import euler_march, euler_step, momentum_march, momentum_step, rk_march, rk_step

DTYPES = [("single", torch.float32), ("double", torch.float64)]


@pytest.mark.parametrize("prec,tdt", DTYPES)
def test_unit_diffusivity_is_the_oracle_laplacian_bit_for_bit(prec, tdt):
    n = [5, 9, 17]
    mesh = O.OMesh([0.0, 0.0, 0.0], [0.25 * (m - 1) for m in n], n, prec)
    assert all(float(d) == 0.25 for d in mesh.dx)
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(3, 0.0, "dirichlet"))
    g = torch.Generator().manual_seed(1)
    phi = torch.randint(-8, 9, (1, *n), generator=g).to(tdt)
    sl = O.interior_slicer(3, bcs)
    lap = O.apply_laplacian(O.laplacian_tables(phi, mesh, bcs), phi, 3)
    d = R.nu_term(phi, torch.ones(n, dtype=tdt), mesh)
    assert d.dtype == tdt
    assert float(lap[0][sl].abs().max()) > 0
    assert torch.equal(d[0][sl], lap[0][sl])
    # and the step with it is the constant-nu step of the oracle with nu = 1 (1 * lap is lap)
    a = R.euler_step(phi, 0.0, torch.ones(n, dtype=tdt), 2.0 ** -10, mesh, bcs, "upwind")
    b = O.euler_step(phi, 0.0, 1.0, 2.0 ** -10, mesh, bcs, "upwind")
    assert torch.equal(a, b)


@pytest.mark.parametrize("prec,tdt", DTYPES)
def test_discrete_steady_state_of_two_materials(prec, tdt):
    n = 17
    mesh = O.OMesh([0.0], [1.0], [n], prec)
    bcs = O.make_bcs(mesh, O.mixed_cfg([0.0, 1.0], ["dirichlet", "dirichlet"], O.FACES[:2]))
    nu64 = torch.ones(n, dtype=torch.float64)
    nu64[8:] = 4.0
    face = 0.5 * (nu64[:-1] + nu64[1:])                       # nu_{i+1/2}
    cum = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(1.0 / face, 0)])
    phi = (cum / cum[-1]).to(tdt).unsqueeze(0)
    nu = nu64.to(tdt)
    assert float(phi[0, 0]) == 0.0 and float(phi[0, -1]) == 1.0
    dt = 1e-4
    new = R.euler_step(phi, 0.0, nu, dt, mesh, bcs, "upwind")
    sl = O.interior_slicer(1, bcs)
    inc = float((new[0][sl] - phi[0][sl]).abs().max())
    eps = float(torch.finfo(tdt).eps)
    x = phi[0].double()
    nup_fp = ((torch.roll(nu64, -1) + nu64) * (torch.roll(x, -1) - x))[sl]
    w = float(R.face_weights(phi[0], mesh)[0])
    bound = 16 * eps * float(nup_fp.abs().max()) * w * dt
    print(f"{prec}: increment {inc:.3e}, bound {bound:.3e}")
    assert inc <= bound
    assert torch.equal(new[0][[0, -1]], phi[0][[0, -1]])      # the fill leaves the dirichlet values


@pytest.mark.parametrize("prec,tdt", DTYPES)
def test_the_step_conserves_the_sum(prec, tdt):
    n = [12, 11, 16]
    mesh = O.OMesh([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], n, prec)
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(3, 0.0, "dirichlet"))
    g = torch.Generator().manual_seed(2)
    phi = torch.zeros((1, *n), dtype=tdt)
    phi[0, 3:9, 3:8, 4:12] = torch.rand((6, 5, 8), generator=g, dtype=torch.float64).to(tdt)
    nu = (0.1 + torch.rand(n, generator=g, dtype=torch.float64)).to(tdt)
    dt = 2e-4
    new = R.euler_step(phi, 0.0, nu, dt, mesh, bcs, "upwind")
    diff = (new - phi).double()
    total, moved = float(diff.sum().abs()), float(diff.abs().sum())
    x, nc = phi[0].double(), nu.double()
    w = R.face_weights(phi[0], mesh)
    flux = sum(float((dt * float(w[a]) * (torch.roll(nc, -1, a) + nc) * (torch.roll(x, -1, a) - x)).abs().sum()) for a in range(3))
    eps = float(torch.finfo(tdt).eps)
    print(f"{prec}: |sum(v - phi)| {total:.3e}, bound {64 * eps * flux:.3e}, ratio to sum|v - phi| {total / moved:.3e}")
    assert moved > 0
    assert total <= 64 * eps * flux


def test_the_restated_march_composes():
    """the stage and the march are march_ref's with this step: order 2 written out once, a source, a velocity and minmod run"""
    n = [6, 7, 9]
    mesh = O.OMesh([0.0] * 3, [1.0] * 3, n, "double")
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(3, 0.25, "dirichlet"))
    g = torch.Generator().manual_seed(4)
    phi = torch.rand((1, *n), generator=g, dtype=torch.float64)
    O.bc_fill(phi, bcs)
    nu = 0.01 + 0.01 * torch.rand(n, generator=g, dtype=torch.float64)
    S = torch.randn((1, *n), generator=g, dtype=torch.float64)
    dt = 1e-3
    e1 = R.euler_step(phi, 0.7, nu, dt, mesh, bcs, "upwind", S)
    want = (0.5 * phi) + (0.5 * R.euler_step(e1, 0.7, nu, dt, mesh, bcs, "upwind", S))
    O.bc_fill(want, bcs)
    assert torch.equal(R.march(phi, 0.7, nu, dt, 1, mesh, bcs, "upwind", 2, S), want)
    assert torch.equal(R.euler_step(phi, 0.7, nu, dt, mesh, bcs), R.euler_step(phi, 0.7, nu.unsqueeze(0), dt, mesh, bcs))
    for limiter, u in (("quick", [0.3, -0.2, 0.5]), ("minmod", 0.7), ("none", 0.7)):
        out = R.march(phi, u, nu, dt, 2, mesh, bcs, limiter, 3)
        assert torch.isfinite(out).all() and not torch.equal(out, phi)


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


def _calls(phi, nu, **kw):
    """the four scalar entry points (rk at orders 1 .. 3) as thunks"""
    out = [lambda: euler_step(phi, 1.0, nu, 1e-3, **kw), lambda: euler_march(phi, 1.0, nu, 1e-3, 2, **kw)]
    for order in (1, 2, 3):
        out.append(lambda order=order: rk_step(phi, 1.0, nu, 1e-3, order=order, **kw))
        out.append(lambda order=order: rk_march(phi, 1.0, nu, 1e-3, 2, order=order, **kw))
    return out


def _vector_calls(U, nu, **kw):
    return [lambda: momentum_step(U, nu, 1e-3, **kw), lambda: momentum_march(U, nu, 1e-3, 2, **kw)]


def test_diffusivity_argument_checks_fire_before_a_device_is_touched():
    from pyapes_amd.geometry import Cylinder
    phi = _cpu_field()
    U = _cpu_field(dim=2)
    shape = phi().shape
    bad_values = [
        torch.ones(1, 9, 8, dtype=torch.float64),           # wrong shape
        torch.ones(9, 8, dtype=torch.float64),
        torch.ones(2, 9, 9, dtype=torch.float64),
        torch.ones(shape, dtype=torch.float32),             # wrong dtype
    ]
    if torch.cuda.is_available():
        bad_values.append(torch.ones(shape, dtype=torch.float64, device="cuda"))   # wrong device
    for bad in bad_values:
        for call in _calls(phi, bad) + _vector_calls(U, bad):
            with pytest.raises(ValueError):
                call()
    for bad in (phi(), phi()[0]):                           # phi's own tensor, a view on its storage
        for call in _calls(phi, bad):
            with pytest.raises(ValueError):
                call()
    for call in _vector_calls(U, U()[1]):                   # a component of the vector that is marched
        with pytest.raises(ValueError):
            call()
    other = _cpu_field()
    for call in _calls(phi, U) + _vector_calls(U, U):       # a vector Field
        with pytest.raises(NotImplementedError):
            call()
    for call in _calls(phi, other) + _vector_calls(U, other):   # a scalar Field, but on another mesh
        with pytest.raises(ValueError):
            call()
    compat = {"div": {"limiter": "upwind", "compat": True}}
    for call in _calls(phi, torch.ones(shape, dtype=torch.float64), config=compat):
        with pytest.raises(NotImplementedError):
            call()
    slab = _cpu_field(n=(9, 9, 9), slab=(0, 2))
    rz = _cpu_field(geo=Cylinder[0:1, 0:1])
    for f in (slab, rz):
        for call in _calls(f, torch.ones(f().shape, dtype=torch.float64)):
            with pytest.raises(NotImplementedError):
                call()


def test_a_good_diffusivity_and_a_number_get_past_the_checks():
    """past the argument checks a CPU mesh fails where it does today: the march itself needs the GPU (RuntimeError, not one of
    the checks' own NotImplementedError)"""
    phi = _cpu_field()
    U = _cpu_field(dim=2)
    from pyapes_amd.variables.bcs import mixed_bcs
    same_mesh = type(phi)("nu", 1, phi.mesh, {"domain": mixed_bcs([0.0] * 4, ["dirichlet"] * 4), "obstacle": None})
    on_U = type(phi)("nu", 1, U.mesh, {"domain": mixed_bcs([0.0] * 4, ["dirichlet"] * 4), "obstacle": None})
    good = [0.05, 1, torch.ones(phi().shape, dtype=torch.float64), torch.ones(9, 9, dtype=torch.float64),
            torch.ones(9, 18, dtype=torch.float64)[:, ::2], same_mesh]
    for nu in good:
        calls = _calls(phi, nu) + _calls(phi, nu, source=1.0) + _calls(phi, nu, config={"div": {"limiter": "quick"}})
        if not isinstance(nu, type(phi)):
            calls += _vector_calls(U, nu)
        for call in calls:
            with pytest.raises(RuntimeError) as ei:
                call()
            assert ei.type is RuntimeError, (nu, ei.value)
    for call in _vector_calls(U, on_U):
        with pytest.raises(RuntimeError) as ei:
            call()
        assert ei.type is RuntimeError
