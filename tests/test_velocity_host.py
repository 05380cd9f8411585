"""No GPU: the marches in a velocity field -- one advection speed per mesh axis -- on the CPU.  The velocity form of
tests/march_ref.py (the step, the stage and the march restated operation for operation as the kernels compute them) against
its one-speed form and the oracle, what the scheme does (an exact shift, a solid-body rotation), and the argument checks of
pyapes_amd/solver/march.py, which fire before a device is touched.

Solid-body rotation (measured on the CPU, printed by the test): a Gaussian of width 0.08 at (0.5, 0.3) on [0, 1]^2, angular
speed 2 pi about the centre, a quarter turn, order 3, nu = 0, dt = 0.2 dx / max|u|, all faces dirichlet 0.  Max-abs error
against the rotated profile at 33^2 / 65^2:
    QUICK   0.0634 / 0.0124  (ratio 5.13, observed order 2.36)
    upwind  0.493 / 0.331    (ratio 1.49, observed order 0.57: first order is not yet asymptotic on a pulse 2.6 / 5 cells wide)
QUICK / upwind: 0.129 at 33^2, 0.037 at 65^2.  Asserted: both errors fall under refinement and QUICK's is below upwind's at both
resolutions -- no figure nobody has derived.
"""
import math

import pytest
import torch

import march_ref as R
import pyapes_oracle as O
from pyapes_amd.solver import march as M
from pyapes_amd.solver.march import euler_march, euler_step, rk_march, rk_step


def _mesh_and_field(n, dtype, seed=3):
    nd = len(n)
    mesh = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(nd, 0.25, "dirichlet"))
    g = torch.Generator().manual_seed(seed)
    tdt = torch.float64 if dtype == "double" else torch.float32
    phi = torch.rand((1, *n), generator=g, dtype=torch.float64).to(tdt)
    O.bc_fill(phi, bcs)
    U = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(tdt)
    return mesh, bcs, phi, U


@pytest.mark.parametrize("limiter", ["upwind", "none", "quick"])
@pytest.mark.parametrize("n,dtype", [([7, 9, 12], "single"), ([7, 9, 12], "double"), ([17, 12], "double"), ([33], "single")],
                         ids=["3d_f32", "3d_f64", "2d_f64", "1d_f32"])
def test_equal_components_are_the_single_speed(n, dtype, limiter):
    """(c, .., c) and (U, .., U): bit-identical to the one-speed march_ref.euler_step, with and without a source"""
    mesh, bcs, phi, U = _mesh_and_field(n, dtype)
    nd = len(n)
    src = torch.randn(phi.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(phi.dtype)
    for c in (0.9, -0.8):
        for s in (None, src, 1.75):
            assert torch.equal(R.euler_step(phi, [c] * nd, 0.05, 1e-3, mesh, bcs, limiter, s),
                               R.euler_step(phi, c, 0.05, 1e-3, mesh, bcs, limiter, s))
    one = U[0:1]
    for s in (None, src):
        assert torch.equal(R.euler_step(phi, [one[0]] * nd, 0.05, 1e-3, mesh, bcs, limiter, s),
                           R.euler_step(phi, one, 0.05, 1e-3, mesh, bcs, limiter, s))
    assert torch.equal(R.march(phi, [one[0]] * nd, 0.05, 1e-3, 2, mesh, bcs, limiter, 3, src),
                       R.march(phi, one, 0.05, 1e-3, 2, mesh, bcs, limiter, 3, src))


# the eight BC sets and the mesh shapes of tests/test_gpu_chunks.py / test_gpu_chunks_terms.py, which use BOTH forms
_D, _N, _S, _P = "dirichlet", "neumann", "symmetry", "periodic"
CHUNK_BCS = {
    "NEUSYM": ([0.0, 0.0, None, None, None, None], [_N, _N, _S, _S, _S, _S]),
    "ALLNEU": ([0.3, -0.2, 0.1, 0.0, -0.4, 0.25], [_N] * 6),
    "MIXED": ([0.5, 0.1, None, 1.0, -0.3, None], [_D, _N, _S, _D, _N, _S]),
    "ALLDIR": ([0.0, 1.0, 0.25, -0.5, 2.0, 0.0], [_D] * 6),
    "YPER": ([0.5, 0.1, None, None, -0.3, None], [_D, _N, _P, _P, _N, _S]),
    "DIRPER": ([0.0, 1.0, None, None, None, None], [_D, _D, _P, _P, _P, _P]),
    "XPER": ([None, None, 0.25, -0.5, 2.0, 0.0], [_P, _P, _D, _D, _D, _D]),
    "ALLPER": ([None] * 6, [_P] * 6),
}


@pytest.mark.parametrize("limiter", ["upwind", "quick", "none"])
@pytest.mark.parametrize("dtype", ["double", "single"])
def test_the_two_references_agree_on_the_chunk_test_meshes(dtype, limiter):
    """with a source field, a stage of march_ref in a velocity of three equal components is its stage with the one speed, bit for
    bit and finite: on the eight BC sets and the row counts / row lengths of the chunk tests (eight-node rows, one- and two-tile rows),
    so that both forms are defined on every input those tests hand them"""
    tdt = torch.float64 if dtype == "double" else torch.float32
    ran = 0
    for n in ([5, 19, 36], [9, 5, 32], [6, 6, 32], [7, 8, 8], [13, 9, 132 if dtype == "double" else 260]):
        for name, (vals, types) in CHUNK_BCS.items():
            if limiter == "none" and any(t in (_N, _S) for t in types):
                continue                                    # central Div is refused on neumann / symmetry faces
            mesh = O.OMesh([0.0] * 3, [1.0] * 3, n, dtype)
            bcs = O.make_bcs(mesh, O.mixed_cfg(list(vals), list(types), O.FACES[:6]))
            g = torch.Generator().manual_seed(17)
            phi, phi0 = (torch.rand((1, *n), generator=g, dtype=torch.float64).to(tdt) for _ in range(2))
            O.bc_fill(phi, bcs)
            O.bc_fill(phi0, bcs)
            U = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
            src = (3.0 * torch.randn((1, *n), generator=g, dtype=torch.float64)).to(tdt)
            dx = 1.0 / (max(n) - 1)
            nu, dt = 1e-3, 0.2 * min(dx * dx / 6e-3, dx / 1.3)
            for u_vel, u_one in (([-0.8] * 3, -0.8), ([U[0]] * 3, U)):
                a = R.rk_stage(phi, phi0, 0.75, 0.25, u_vel, nu, dt, mesh, bcs, limiter, src)
                b = R.rk_stage(phi, phi0, 0.75, 0.25, u_one, nu, dt, mesh, bcs, limiter, src)
                assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (n, name)
                ran += 1
    assert ran == (40 if limiter == "none" else 80)


@pytest.mark.parametrize("n,dtype", [([7, 9, 12], "single"), ([7, 9, 12], "double"), ([17, 12], "double")],
                         ids=["3d_f32", "3d_f64", "2d_f64"])
def test_upwind_is_the_oracle_on_the_stacked_field(n, dtype):
    """the oracle's own per-axis indexing: adv[a] and var[a] on axis a of a field with mesh.dim components"""
    mesh, bcs, phi, U = _mesh_and_field(n, dtype)
    nd = len(n)
    stacked = phi[0].unsqueeze(0).repeat(nd, *([1] * nd))
    want = O.div_upwind_intended(U, stacked, mesh)
    got = R.adv_upwind([U[a] for a in range(nd)], phi, mesh)
    assert torch.equal(got, want)
    mixed = [0.9, -0.8, 0.4][:nd]
    filled = torch.stack([torch.full_like(phi[0], v) for v in mixed])
    assert torch.equal(R.adv_upwind(mixed, phi, mesh), O.div_upwind_intended(filled, stacked, mesh))
    # distinct components: swapping two axes' speeds is another operator
    swapped = [U[1], U[0]] + [U[a] for a in range(2, nd)]
    assert not torch.equal(R.adv_upwind(swapped, phi, mesh), want)


def shift_case(dtype):
    """dx = 1 on every axis, small integers, dirichlet faces: (oracle mesh, BCs, field)"""
    n = [9, 14, 132]
    mesh = O.OMesh([0.0, 0.0, 0.0], [8.0, 13.0, 131.0], n, dtype)
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(3, 2.0, "dirichlet"))
    g = torch.Generator().manual_seed(7)
    tdt = torch.float64 if dtype == "double" else torch.float32
    phi = torch.randint(-8, 9, (1, *n), generator=g).to(tdt)
    O.bc_fill(phi, bcs)
    return mesh, bcs, phi


@pytest.mark.parametrize("dtype", ["single", "double"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_exact_shift(axis, dtype):
    """u = +e_a: one upwind Euler step with dt = dx = 1, nu = 0 IS the field shifted by one node along a, exactly; -e_a: the
    other way"""
    mesh, bcs, phi = shift_case(dtype)
    sl = O.interior_slicer(3, bcs)
    for sign in (1.0, -1.0):
        u = [0.0, 0.0, 0.0]
        u[axis] = sign
        got = R.euler_step(phi, u, 0.0, 1.0, mesh, bcs, "upwind")
        want = torch.roll(phi[0], 1 if sign > 0 else -1, axis)
        assert torch.equal(got[0][sl], want[sl]), (axis, sign)
        ut = [torch.full_like(phi[0], v) for v in u]
        assert torch.equal(R.euler_step(phi, ut, 0.0, 1.0, mesh, bcs, "upwind"), got)


def _rotation_error(N, limiter):
    mesh = O.OMesh([0.0, 0.0], [1.0, 1.0], [N, N], "double")
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(2, 0.0, "dirichlet"))
    x, y = mesh.grid
    w = 2.0 * math.pi

    def pulse(cx, cy):
        return torch.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * 0.08 ** 2)).unsqueeze(0)

    phi = pulse(0.5, 0.3)
    O.bc_fill(phi, bcs)
    u = [-w * (y - 0.5), w * (x - 0.5)]            # counter-clockwise about the centre
    T = 0.25                                        # a quarter turn: (0.5, 0.3) -> (0.7, 0.5)
    dx = 1.0 / (N - 1)
    nsteps = int(math.ceil(T / (0.2 * dx / (w * 0.5 * math.sqrt(2.0)))))
    end = R.march(phi, u, 0.0, T / nsteps, nsteps, mesh, bcs, limiter, 3)
    return float((end - pulse(0.7, 0.5)).abs().max())


def test_solid_body_rotation():
    err = {lim: [_rotation_error(N, lim) for N in (33, 65)] for lim in ("quick", "upwind")}
    for lim, (e1, e2) in err.items():
        print(f"rotation {lim}: max error 33^2 {e1:.4g}, 65^2 {e2:.4g}, ratio {e1 / e2:.3f}, observed order {math.log2(e1 / e2):.2f}")
    print(f"rotation quick / upwind: 33^2 {err['quick'][0] / err['upwind'][0]:.3f}, 65^2 {err['quick'][1] / err['upwind'][1]:.3f}")
    for lim in err:
        assert err[lim][1] < err[lim][0], err
    for q, p in zip(err["quick"], err["upwind"]):
        assert q < p, err


# ---- the checks in front of the device -------------------------------------------------------------------------------
def _cpu_field(n=(9, 9), dim=1, slab=None, geo=None):
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    box = geo if geo is not None else (Box[0:1] if len(n) == 1 else (Box[0:1, 0:1] if len(n) == 2 else Box[0:1, 0:1, 0:1]))
    kw = {"slab": slab} if slab else {}
    mesh = Mesh(box, None, list(n), "cpu", "double", **kw)
    cfg = mixed_bcs([0.0] * (2 * len(n)), ["dirichlet"] * (2 * len(n)))
    if geo is not None:
        cfg = [dict(c, bc_face=f) for c, f in zip(cfg, O.FACES_RZ)]
    return Field("phi", dim, mesh, {"domain": cfg, "obstacle": None})


def _calls(phi, u, **kw):
    out = [lambda: euler_step(phi, u, 0.05, 1e-3, **kw), lambda: euler_march(phi, u, 0.05, 1e-3, 2, **kw)]
    for order in (1, 2, 3):
        out.append(lambda order=order: rk_step(phi, u, 0.05, 1e-3, order=order, **kw))
        out.append(lambda order=order: rk_march(phi, u, 0.05, 1e-3, 2, order=order, **kw))
    return out


@pytest.fixture
def no_device(monkeypatch):
    """a refusal must come before context_for (and before require_gpu) is reached"""
    def reached(*a, **k):
        raise AssertionError("a device was touched before the velocity was checked")
    monkeypatch.setattr(M, "context_for", reached)
    monkeypatch.setattr(M, "require_gpu", reached)


def test_velocity_argument_checks_fire_before_a_device_is_touched(no_device):
    from pyapes_amd.geometry import Cylinder
    phi = _cpu_field()
    comp = phi()[0].shape
    good = torch.zeros(comp, dtype=torch.float64)
    refusals = [
        ((1.0,), ValueError),                                               # wrong number of entries
        ([1.0, 2.0, 3.0], ValueError),
        ((good, torch.zeros(9, 8, dtype=torch.float64)), ValueError),       # wrong shape
        ((torch.zeros(1, 9, 9, dtype=torch.float64), 1.0), ValueError),
        ((good, torch.zeros(comp, dtype=torch.float32)), ValueError),       # wrong dtype
        ((phi()[0], 1.0), ValueError),                                      # a component on phi's storage
        ((good, "fast"), TypeError),
        ((True, 1.0), TypeError),
        (_cpu_field(dim=2), ValueError),                                    # a vector Field on another mesh
    ]
    refusals.append(((good, torch.zeros(comp, dtype=torch.float64, device="meta")), ValueError))       # wrong device
    for u, exc in refusals:
        for call in _calls(phi, u):
            with pytest.raises(exc):
                call()
    for call in _calls(phi, (1.0, 2.0), config={"div": {"limiter": "upwind", "compat": True}}):
        with pytest.raises(NotImplementedError):
            call()
    slab = _cpu_field(n=(9, 9, 9), slab=(0, 2))
    for u in ((1.0, 2.0, 3.0), torch.zeros((3, 9, 9, 9), dtype=torch.float64)):
        for call in _calls(slab, u):
            with pytest.raises(NotImplementedError):
                call()
    rz = _cpu_field(geo=Cylinder[0:1, 0:1])
    for call in _calls(rz, (1.0, 2.0)):
        with pytest.raises(NotImplementedError):
            call()
    vec = _cpu_field(dim=2)                                                 # phi must be a scalar field
    for call in _calls(vec, (1.0, 2.0)):
        with pytest.raises(NotImplementedError):
            call()


def test_a_good_velocity_gets_past_the_checks(monkeypatch):
    """every accepted form arrives at the Context as the per-axis list ``_velocity_of`` makes of it: the march's own
    ``context_for`` is replaced by a recorder (a CPU mesh has no device to ask)"""
    phi = _cpu_field()
    from pyapes_amd.variables.bcs import mixed_bcs
    comp = phi()[0].shape
    t = torch.arange(81, dtype=torch.float64).reshape(comp)
    t2 = -t.clone()
    vecf = type(phi)("u", 2, phi.mesh, {"domain": mixed_bcs([0.0] * 4, ["dirichlet"] * 4), "obstacle": None})
    vecf.set_var_tensor(torch.stack([t, t2]))
    seen = []

    class Recorder:
        def bind_bcs(self, *a, **k):
            pass

        def euler_step_vel(self, phi_, out, kind, vel, nu, dt, source=None):
            seen.append((vel, source))
            out.copy_(phi_)

        def rk_march_vel(self, phi_, w1, w2, order, kind, vel, nu, dt, nsteps, source=None):
            seen.append((vel, source))
            return phi_

        def __getattr__(self, name):   # a one-speed entry point: the velocity was not recognised
            raise AssertionError(f"a velocity went to Context.{name}")

    monkeypatch.setattr(M, "context_for", lambda mesh: Recorder())
    monkeypatch.setattr(M, "require_gpu", lambda *a, **k: None)

    def same(got, want):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            if isinstance(w, torch.Tensor):
                assert isinstance(g, torch.Tensor) and g.is_contiguous() and torch.equal(g, w)
            else:
                assert isinstance(g, float) and g == w

    forms = [((1.0, -2.0), [1.0, -2.0]), ([1, 0.5], [1.0, 0.5]), ((t, 2.0), [t, torch.full_like(t, 2.0)]), ((t, t2), [t, t2]),
             (torch.stack([t, t2]), [t, t2]), (vecf, [t, t2]), ((t.t().contiguous().t(), t2), [t, t2])]
    for u, want in forms:
        for src in (None, 1.5):
            del seen[:]
            calls = _calls(phi, u) if src is None else _calls(phi, u, source=src)
            for call in calls:
                call()
            assert len(seen) == len(calls)
            for vel, source in seen:
                same(vel, want)
                assert source == src
    one_d = _cpu_field(n=(9,))
    del seen[:]
    for call in _calls(one_d, (1.0,)):
        call()
    assert seen and all(vel == [1.0] for vel, _ in seen)
    # one speed for every axis never takes the velocity entry points
    for u in (1.0, torch.ones(phi().shape, dtype=torch.float64)):
        with pytest.raises(AssertionError, match="a velocity went to|Context"):
            euler_step(phi, u, 0.05, 1e-3)


def test_mixed_entries_become_filled_tensors():
    phi = _cpu_field()
    t = torch.ones(phi()[0].shape, dtype=torch.float64)
    v = M._velocity_of(phi, (t, -0.5), None, "euler_step")
    assert all(isinstance(e, torch.Tensor) for e in v) and torch.equal(v[1], torch.full_like(t, -0.5))
    assert M._velocity_of(phi, (1, -0.5), None, "euler_step") == [1.0, -0.5]      # all numbers: scalars down to the kernel
    for one_speed in (1.0, torch.ones(phi().shape, dtype=torch.float64), phi):    # today's forms are not a velocity
        assert M._velocity_of(phi, one_speed, None, "euler_step") is None
