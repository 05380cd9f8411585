"""No GPU: the projection kernels restated on the CPU (tests/projection_ref.py) against an independent float64 formula, the
telescoping sum of the divergence, the fraction of a mode's divergence that the approximate projection leaves, and the argument
checks of ``divergence`` / ``project`` / ``ns_step`` (pyapes_amd/solver/projection.py), which fire before a device is touched.

The fraction (DESIGN.md section 4 "Projection").  On a uniform square mesh take a mode whose phase advances by theta per node on
both axes.  The central difference has the symbol i sin(theta) / h, so divergence after gradient is the WIDE Laplacian,
-(2 sin^2(theta)) / h^2, while the solve inverts the compact one, -(2 * 4 sin^2(theta / 2)) / h^2.  With p = L_compact^-1 (rho/dt) D.U,
    D.(U - (dt/rho) G p) = (1 - L_wide / L_compact) D.U = (1 - sin^2(theta) / (4 sin^2(theta/2))) D.U = sin^2(theta / 2) D.U
since sin^2(theta) = 4 sin^2(theta/2) cos^2(theta/2).  theta = pi / 4 gives  sin^2(pi / 8) = (1 - cos(pi/4)) / 2 = (2 - sqrt 2) / 4.

Where it is measured.  The natural place is a fully periodic mesh.  This tree's periodic layout does not carry a Fourier mode: the
periodic fill rewrites x[0] = x[1] - x[n-1] + x[n-2] and x[n-1] = x[0] after every CG update without the residual knowing, and
the oracle's CG does not converge there (measured on the CPU: on 16^2 .. 65^2 fully periodic meshes it runs into max_it = 2000 or
stops with ratios between 0.29 and 80 where sin^2(theta/2) is 0.04 .. 0.17).  The same derivation holds, node for node, in a
WALLED box: p = 0 (Dirichlet) on every face and the sine mode sin(theta i) sin(theta j), theta = m pi / (N - 1), which is an
eigenvector of the compact Dirichlet Laplacian on the interior set; U = (cos sin, 1/2 sin cos) holds the mode's own values on
its Dirichlet faces.  The BC fill keeps the UNCORRECTED values on the faces, so the first interior layer sees a mismatch: the
ratio is taken over the nodes at least two from a wall, where every stencil involved reads corrected interior values only.
There the CPU chain gives 0.14644660940672638 (fp64) against (2 - sqrt 2) / 4 = 0.14644660940672624.

The telescoping sum needs no substitute: the divergence wraps around like ``torch.roll``, whatever the fill does.
"""
import math

import numpy as np
import pytest
import torch

import projection_ref as PR
import pyapes_oracle as O
from projection_ref import MIXED_TYPES, REMAINING_FRACTION, cpu_field as _cpu_field, eps_of, interior_mask, smooth_vector
from pyapes_amd.solver import march as M
from pyapes_amd.solver import projection as P

MODE_N, MODE_M, MODE_DT, MODE_RHO = PR.MODE_N, PR.MODE_M, PR.MODE_DT, PR.MODE_RHO


def periodic_cfg(nd):
    return O.mixed_cfg([None] * (2 * nd), ["periodic"] * (2 * nd), O.FACES[:2 * nd])


# ---- the restatement against an independent formula -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("n", [[11, 13], [7, 9, 12]], ids=["2d", "3d"])
def test_restatement_against_a_float64_formula(n, dtype):
    """numpy, float64, the textbook expressions: (U_a[+1] - U_a[-1]) / (2 dx_a) summed, U_c - scale (p[+1] - p[-1]) / (2 dx_c).
    Bound: every operand is rounded to the dtype (eps / 2 relative each), and the restatement rounds the difference, the
    product with h_a (itself rounded), the sum and the product with the scale: at most 6 roundings on the way of any operand
    pair, so |error| <= 6 eps (|U[+1]| + |U[-1]|) h_a per axis (3 eps would be the first-order count; 6 leaves room for the
    second-order terms and the rounded scale), times |scale|.  In fp64 the inputs are exact and the bound is not tight."""
    nd = len(n)
    om = O.OMesh([0.0] * nd, [1.0, 1.5, 0.75][:nd], list(n), dtype)
    types = MIXED_TYPES[-2 * nd:] if nd == 2 else MIXED_TYPES
    vals = [None if t in ("symmetry", "periodic") else 0.25 for t in types]
    bcs = O.make_bcs(om, O.mixed_cfg(vals, types, O.FACES[:2 * nd]))
    U64, p64 = smooth_vector(om)
    U = torch.from_numpy(U64).to(om.dtype)
    p = torch.from_numpy(p64).to(om.dtype).unsqueeze(0)
    dx = [float(om.dx[a]) for a in range(nd)]
    eps = eps_of(om.dtype)
    inside = interior_mask(om, bcs)
    for scale in (1.0, 1.0 / 0.003, -0.75):
        want = sum((np.roll(U64[a], -1, a) - np.roll(U64[a], 1, a)) / (2.0 * dx[a]) for a in range(nd)) * scale
        bound = sum((np.abs(np.roll(U64[a], -1, a)) + np.abs(np.roll(U64[a], 1, a))) / (2.0 * dx[a]) for a in range(nd))
        got = PR.divergence(U, om, bcs, scale)
        assert got.shape == (1, *n) and got.dtype == om.dtype
        g = got[0].double().numpy()
        assert np.all(g[~inside] == 0.0) and not np.any(np.signbit(g[~inside]))
        assert np.all(np.abs(g - want)[inside] <= 6.0 * eps * abs(scale) * bound[inside]), (scale, np.abs(g - want)[inside].max())
        out = PR.correct(U, p, om, bcs, scale, fill=False).double().numpy()
        for c in range(nd):
            grad = (np.roll(p64, -1, c) - np.roll(p64, 1, c)) / (2.0 * dx[c])
            gb = (np.abs(np.roll(p64, -1, c)) + np.abs(np.roll(p64, 1, c))) / (2.0 * dx[c])
            tol = 6.0 * eps * (abs(scale) * gb + np.abs(U64[c]))
            assert np.all(np.abs(out[c] - (U64[c] - scale * grad))[inside] <= tol[inside]), (scale, c)
            assert np.array_equal(out[c][~inside], U[c].double().numpy()[~inside])
    # the fill behind the correction is the oracle's, component by component
    filled = PR.correct(U, p, om, bcs, 0.5)
    assert torch.equal(filled, O.bc_fill(PR.correct(U, p, om, bcs, 0.5, fill=False), bcs))


def test_the_restatement_rounds_every_operation_in_the_dtype():
    """fp32: the restated divergence is NOT the float64 formula rounded once (it would be, were an operation carried out in
    double), and the scale is applied to the finished sum"""
    om = O.OMesh([0.0, 0.0], [1.0, 1.0], [11, 13], "single")
    bcs = O.make_bcs(om, periodic_cfg(2))
    g = torch.Generator().manual_seed(3)
    U = torch.randn((2, 11, 13), generator=g, dtype=torch.float64).to(torch.float32)
    h = PR.half_inverse_spacing(om, torch.float32)
    d0 = (torch.roll(U[0], -1, 0) - torch.roll(U[0], 1, 0)) * h[0]
    d1 = (torch.roll(U[1], -1, 1) - torch.roll(U[1], 1, 1)) * h[1]
    want = torch.tensor(-3.7, dtype=torch.float32) * ((torch.zeros_like(d0) + d0) + d1)
    assert torch.equal(PR.divergence(U, om, bcs, -3.7)[0], want)
    once = (-3.7 * ((torch.roll(U[0].double(), -1, 0) - torch.roll(U[0].double(), 1, 0)) * (0.5 / float(om.dx[0]))
                    + (torch.roll(U[1].double(), -1, 1) - torch.roll(U[1].double(), 1, 1)) * (0.5 / float(om.dx[1])))).float()
    assert not torch.equal(want, once)


# ---- telescoping ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", [([16, 16, 32], "double"), ([11, 13], "single"), ([9, 10, 11], "single")],
                         ids=["3d_f64", "2d_f32", "3d_f32"])
def test_the_divergence_of_a_periodic_mesh_sums_to_zero(n, dtype):
    """fully periodic: the interior set is every node and every U_a[+1] is some other node's U_a[-1], so the exact sum is 0.
    What is left is the rounding of the cells: per cell and axis the difference and the product with h_a (2 roundings, h_a
    itself rounded: 3), then the running sum (one per axis, on a partial sum no larger than the terms so far), so
    |sum| <= sum over cells of  (3 + nd) eps * sum_a (|U_a[+1]| + |U_a[-1]|) h_a,  the cells added up in double."""
    nd = len(n)
    om = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
    bcs = O.make_bcs(om, periodic_cfg(nd))
    g = torch.Generator().manual_seed(1)
    U = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(om.dtype)
    O.bc_fill(U, bcs)
    d = PR.divergence(U, om, bcs)[0].double()
    h = [0.5 / float(om.dx[a]) for a in range(nd)]
    mag = sum((torch.roll(U[a], -1, a).abs() + torch.roll(U[a], 1, a).abs()).double() * h[a] for a in range(nd))
    bound = (3 + nd) * eps_of(om.dtype) * float(mag.sum())
    print(f"telescoping {n} {dtype}: sum {float(d.sum()):.3e}, sum of |cells| {float(d.abs().sum()):.3e}, bound {bound:.3e}")
    assert float(d.abs().sum()) > 1e3 * bound      # the cells themselves are far from zero
    assert abs(float(d.sum())) <= bound


# ---- the approximate projection leaves sin^2(theta / 2) of a mode's divergence --------------------------------------
@pytest.mark.parametrize("dtype", ["double", "single"])
def test_projection_leaves_the_derived_fraction_of_a_mode(dtype):
    """the walled single-mode problem of the module docstring (projection_ref.mode_case)"""
    assert MODE_M * 4 == MODE_N - 1            # theta = pi / 4
    om, U, face_vals = PR.mode_case(dtype)
    ubcs = O.make_bcs(om, O.mixed_cfg(face_vals, ["dirichlet"] * 4, O.FACES[:4]))
    pcfg = O.mixed_cfg([0.0] * 4, ["dirichlet"] * 4, O.FACES[:4])
    before = PR.divergence(U, om, ubcs)
    tol = 1e-13 if dtype == "double" else 1e-7
    U1, p1, rep = PR.project(U, torch.zeros((1, MODE_N, MODE_N), dtype=om.dtype), MODE_DT, MODE_RHO, om, ubcs, pcfg, tol, 500)
    ratio = PR.inner_norm(PR.divergence(U1, om, ubcs)) / PR.inner_norm(before)
    print(f"projection of a mode, {dtype}: itr {rep['itr']}, ratio {ratio!r}, derived {REMAINING_FRACTION!r}")
    assert rep["itr"] < 500
    assert abs(REMAINING_FRACTION - math.sin(math.pi / 8.0) ** 2) < 1e-15
    # the suite's solver tolerances, relative
    assert abs(ratio - REMAINING_FRACTION) <= (1e-10 if dtype == "double" else 1e-5) * REMAINING_FRACTION
    # and the remainder is the mode itself, scaled: not rounding, not zero
    assert ratio > 0.1


# ---- the checks in front of the device ------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """a refusal must come before context_for (and before require_gpu) is reached, in this module and in the march's"""
    def reached(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    for mod in (P, M):
        monkeypatch.setattr(mod, "context_for", reached)
        monkeypatch.setattr(mod, "require_gpu", reached)


def _calls(U, p, dt=1e-3, rho=1.0):
    return [lambda: P.project(U, p, dt, rho), lambda: P.project(U, p, dt, rho=rho, solver={"fdm": {"method": "cg"}}),
            lambda: P.ns_step(U, p, 0.05, dt, rho=rho), lambda: P.ns_step(U, p, 0.05, dt, None, 2, rho=rho)]


def test_argument_checks_fire_before_a_device_is_touched(no_device):
    from pyapes_amd.geometry import Cylinder
    U = _cpu_field()
    p = _cpu_field(dim=1, name="p", mesh=U.mesh)
    # the velocity: slab, rz, 1-D, U.dim != mesh.dim -- on all three entry points
    for bad in (_cpu_field(n=(9, 9, 9), slab=(0, 2)), _cpu_field(geo=Cylinder[0:1, 0:1]), _cpu_field(n=(9,)),
                _cpu_field(dim=1), _cpu_field(dim=3), _cpu_field(n=(9, 9, 9), dim=2)):
        bp = _cpu_field(dim=1, name="p", mesh=bad.mesh)
        for call in [lambda: P.divergence(bad), lambda: P.divergence(bad, 2.0)] + _calls(bad, bp):
            with pytest.raises(NotImplementedError):
                call()
    for notfield in (U(), None, 1.0):
        for call in [lambda: P.divergence(notfield)] + _calls(notfield, p):
            with pytest.raises(TypeError):
                call()
    # p: a scalar Field on U's mesh, of U's dtype and device
    for notp in (p(), None, _cpu_field(dim=2, name="p", mesh=U.mesh)):
        for call in _calls(U, notp):
            with pytest.raises(TypeError):
                call()
    other = _cpu_field(dim=1, name="p")
    for call in _calls(U, other):
        with pytest.raises(ValueError, match="another mesh"):
            call()
    p32 = _cpu_field(dim=1, name="p", mesh=U.mesh)
    p32.set_var_tensor(torch.zeros(p().shape, dtype=torch.float32))
    for call in _calls(U, p32):
        with pytest.raises(ValueError, match="dtype"):
            call()
    pmeta = _cpu_field(dim=1, name="p", mesh=U.mesh)
    pmeta.set_var_tensor(torch.zeros(p().shape, dtype=torch.float64, device="meta"))
    for call in _calls(U, pmeta):
        with pytest.raises(ValueError, match=" on "):
            call()
    # dt and rho: positive numbers
    for dt, rho in ((0.0, 1.0), (-1e-3, 1.0), (1e-3, 0.0), (1e-3, -2.0), (float("nan"), 1.0), (1e-3, float("nan"))):
        for call in _calls(U, p, dt, rho):
            with pytest.raises(ValueError):
                call()
    for dt, rho in (("fast", 1.0), (None, 1.0), (True, 1.0), (1e-3, "heavy"), (1e-3, None), (1e-3, False)):
        for call in _calls(U, p, dt, rho):
            with pytest.raises(TypeError):
                call()
    # divergence: scale a number, out a tensor of the mesh's shape, dtype and device
    for scale in ("big", None, True):
        with pytest.raises(TypeError):
            P.divergence(U, scale)
    comp = tuple(U()[0].shape)
    for out in (torch.zeros(2, *comp, dtype=torch.float64), torch.zeros(9, 8, dtype=torch.float64),
                torch.zeros(comp, dtype=torch.float32), torch.zeros(comp, dtype=torch.float64, device="meta"), [0.0]):
        with pytest.raises(ValueError):
            P.divergence(U, 1.0, out)
    # ns_step: the momentum step's own refusals arrive before the device too
    with pytest.raises(ValueError):
        P.ns_step(U, p, 0.05, 1e-3, order=4)
    with pytest.raises(NotImplementedError):
        P.ns_step(U, p, 0.05, 1e-3, {"div": {"limiter": "upwind", "compat": True}})


def test_good_arguments_reach_the_device():
    """with every check passed the first thing each entry point asks for is the GPU (a CPU mesh: the backend's refusal)"""
    U = _cpu_field()
    p = _cpu_field(dim=1, name="p", mesh=U.mesh)
    for call in [lambda: P.divergence(U), lambda: P.divergence(U, 2, torch.zeros(tuple(U()[0].shape), dtype=torch.float64))] \
            + _calls(U, p, 1, 2):
        with pytest.raises(RuntimeError, match="GPU|cuda|HIP"):
            call()


def test_the_module_is_part_of_the_package_surface():
    import pyapes_amd
    assert "solver.projection" in pyapes_amd._SUBMODULES
    from pyapes_amd.hip import lib as L
    for name in ("pa_divergence", "pa_project_correct"):
        assert name in L.SIGNATURES
