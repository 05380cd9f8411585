"""No GPU: the slope-limited (TVD) advection schemes, Div limiters "minmod" and "mc", restated on the CPU in tests/march_ref.py, and
the host-side checks in front of the device.

1. With L == 0 the term is march_ref's first-order upwind term, bit for bit.
2. Linear data 1 + 2x - y + 3z on 9 x 11 x 13: all four differences equal the slope, L returns it, the correction vanishes --
   exact at every interior node, the fallback nodes included (bound 1e-12: rounding of O(10) operations on O(10) values).
3. Where the fallback sits, pinned with a cubic on 9 nodes of [0, 1] and minmod.  x^3 is convex and increasing, so the limited
   half picks the smaller (upwind-side) differences: with u = -1, fq = (dp + dm) / 2 -- central, error dx^2 x'''/6 = dx^2 -- at
   i = 1 .. 6 and fq = dp -- first-order, error (x8^3 - x7^3)/dx - 3 x7^2 = 22 dx^2 -- at i = 7 = N - 2 (the fallback one node
   further in would give 19 dx^2 at i = 6; no fallback at i = 7 would read the wrapped x[+2]).  The mirrored cubic (1 - x)^3
   with u = +1 gives the mirrored errors: dx^2 at i = 2 .. 7, 22 dx^2 at i = 1.  On a periodic axis nothing falls back:
   tvd_halves with and without the periodic flag differ at most in bq at index <= 1 and in fq at index >= N - 2.
4. mc is minmod(2 minmod(a, b), (a + b) / 2) on the reference's golden pairs (tests/golden/rfp_rz_*.npz: mc_a, mc_b, mc).
5. The periodic ring: N nodes of the unit interval that wrap around (no BC fill, no diffusion: the definition alone),
   E(x) = x + dt * (-adv), the stages of SSP_STAGES.  Square wave 1 on [N/4, N/2), 64 nodes, 100 steps: the total variation
   sum |x[i+1] - x[i]| does not grow by more than 64 ulp of its value per step, and 0 <= x <= 1 holds exactly, for orders 1 and
   3 at CFL 0.25 and 0.5, order 3 at CFL 0.75, both signs of u, fp64 and fp32 (bounds); QUICK leaves [0, 1] by more than 0.05
   on the same input.
6. Exact bounds 0 <= phi <= 1 through march_ref.march (Laplacian with nu = 0, BC fill with zero dirichlet walls): the
   12 x 14 x 16 block case and the 33^2 solid-body rotation, fp64 and fp32.
7. Gaussian exp(-((x - 0.5) / 0.08)^2) once round the ring, order 3, CFL 0.4, 64 / 128 / 256 nodes: the L1 errors fall under
   refinement and mc < minmod < upwind at every size.
8. The refusals of the Python layer, each before a device is touched.
"""
import glob
import os

import numpy as np
import pytest
import torch

import march_ref as Q
import pyapes_oracle as O

from pyapes_amd.hip import lib as L
from pyapes_amd.solver import march as M
from pyapes_amd.solver.fdc import FDC, div_kind, quick_explicit_only, quick_mesh_check
from pyapes_amd.solver.march import (SSP_STAGES, euler_march, euler_step, momentum_march, momentum_step, rk_march, rk_step)

LIMITERS = ("minmod", "mc")
CONFIG = {lim: {"div": {"limiter": lim}} for lim in LIMITERS}


def test_the_kinds():
    assert L.OP_DIV_MINMOD == 6 and L.OP_DIV_MC == 7
    assert div_kind("minmod", False) == 6 and div_kind("mc", False) == 7
    for lim in LIMITERS:
        with pytest.raises(ValueError, match=lim):
            div_kind(lim, True)
    assert Q.SSP_STAGES == SSP_STAGES


# ---- 1 .. 4: the term ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["double", "single"])
def test_without_a_slope_the_term_is_upwind_bit_for_bit(dtype):
    mesh = O.OMesh([0.0] * 3, [1.0] * 3, [7, 9, 12], dtype)
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(3, 0.0, "dirichlet"))
    g = torch.Generator().manual_seed(2)
    phi = torch.randn((1, 7, 9, 12), generator=g, dtype=torch.float64).to(mesh.dtype)
    u = torch.randn((1, 7, 9, 12), generator=g, dtype=torch.float64).to(mesh.dtype)
    vel = [torch.randn((7, 9, 12), generator=g, dtype=torch.float64).to(mesh.dtype) for _ in range(3)]
    for speed in (0.7, -1.3, u):
        assert torch.equal(Q.div_tvd(speed, phi, mesh, bcs, Q.no_slope), O.div_upwind_intended(speed, phi, mesh))
    assert torch.equal(Q.adv_tvd(vel, phi, mesh, bcs, Q.no_slope), Q.adv_upwind(vel, phi, mesh))
    for lim in LIMITERS:   # and with a slope it is another operator
        assert not torch.equal(Q.div_tvd(u, phi, mesh, bcs, lim), O.div_upwind_intended(u, phi, mesh))


@pytest.mark.parametrize("lim", LIMITERS)
@pytest.mark.parametrize("u", [1.3, -0.7])
def test_linear_data_is_exact(u, lim):
    mesh = O.OMesh([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [9, 11, 13], "double")
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(3, 0.0, "dirichlet"))
    x, y, z = mesh.grid
    phi = (1 + 2 * x - y + 3 * z).unsqueeze(0)
    S = (slice(1, -1),) * 3
    err = float((Q.div_tvd(u, phi, mesh, bcs, lim)[0] - u * (2 - 1 + 3))[S].abs().max())
    print(f"linear u={u} {lim}: max error {err:.3e}")
    assert err <= 1e-12


def test_cubic_error_pins_the_fallback():
    mesh = O.OMesh([0.0], [1.0], [9], "double")
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(1, 0.0, "dirichlet"))
    x = mesh.grid[0]
    dx = mesh.dx_list[0]
    d2 = dx * dx
    hi = (Q.div_tvd(-1.0, (x ** 3).unsqueeze(0), mesh, bcs, "minmod")[0] - (-3 * x * x)).abs()
    lo = (Q.div_tvd(1.0, ((1 - x) ** 3).unsqueeze(0), mesh, bcs, "minmod")[0] - (-3 * (1 - x) ** 2)).abs()
    print("cubic, u = -1:", hi.tolist(), " mirrored, u = +1:", lo.tolist())
    for i in range(1, 7):
        assert abs(float(hi[i]) - d2) <= 1e-12, (i, float(hi[i]))
        assert abs(float(lo[8 - i]) - d2) <= 1e-12, (8 - i, float(lo[8 - i]))
    assert abs(float(hi[7]) - 22 * d2) <= 1e-12, float(hi[7])
    assert abs(float(lo[1]) - 22 * d2) <= 1e-12, float(lo[1])


@pytest.mark.parametrize("lim", LIMITERS)
def test_the_fallback_sits_on_non_periodic_axes_only(lim):
    g = torch.Generator().manual_seed(4)
    x = torch.randn((8, 9, 10), generator=g, dtype=torch.float64)
    for a in range(3):
        n = x.shape[a]
        bq, fq, dm, dp = Q.tvd_halves(x, a, False, lim)
        bqp, fqp, _, _ = Q.tvd_halves(x, a, True, lim)
        idx = torch.arange(n).reshape([n if q == a else 1 for q in range(3)]).expand(x.shape)
        assert torch.equal(bq[idx <= 1], dm[idx <= 1]) and torch.equal(fq[idx >= n - 2], dp[idx >= n - 2])
        assert torch.equal(bq[idx > 1], bqp[idx > 1]) and torch.equal(fq[idx < n - 2], fqp[idx < n - 2])
        # random data: the limited halves at the fallback positions are something else
        assert not torch.equal(bqp[idx <= 1], dm[idx <= 1]) and not torch.equal(fqp[idx >= n - 2], dp[idx >= n - 2])


def test_mc_on_the_golden_pairs():
    files = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "rfp_rz_*.npz")))
    seen = 0
    for f in files:
        g = np.load(f)
        if "mc" not in g.files:
            continue
        a, b, want = (torch.as_tensor(g[k]) for k in ("mc_a", "mc_b", "mc"))
        assert torch.equal(Q.mc(a, b), want), f
        assert torch.equal(Q.minmod(2 * Q.minmod(a, b), (a + b) / 2), want), f
        assert torch.equal(Q.minmod(a, b), O.minmod(a, b)) and torch.equal(Q.mc(a, b), O.mc_limiter(a, b)), f
        m = Q.minmod(a, b)   # the three branches and the zero case all occur
        assert bool(((a >= 0) & (b >= 0) & (m > 0)).any()) and bool(((a < 0) & (b < 0) & (m < 0)).any()) and bool((a * b <= 0).any())
        seen += 1
    assert seen >= 2


# ---- 5, 7: the periodic ring -----------------------------------------------------------------------------------------
class _Ring:
    """N nodes of the unit interval that wrap around: dx = 1 / N"""
    dim = 1

    def __init__(self, n, dtype):
        self.dx = torch.tensor([1.0 / n], dtype=dtype)


def _ring_adv(x, u, ring, scheme):
    uc = torch.full_like(x, float(u))
    zeros = torch.zeros_like(x)
    up, um = torch.max(uc, zeros), torch.min(uc, zeros)
    out = torch.zeros_like(x)
    if scheme == "quick":
        return out + Q.quick_term(x, up, um, 0, True, ring)
    return out + Q.tvd_term(x, up, um, 0, True, ring, Q.no_slope if scheme == "upwind" else scheme)


def ring_march(x, u, dt, nsteps, scheme, order, each=None):
    """the march of tests/march_ref.py on the ring: E(x) = x + dt * (0 - adv), the fused stages c0 x0 + c1 E(x)"""
    ring = _Ring(x.shape[0], x.dtype)

    def E(v):
        a = torch.zeros_like(v) - _ring_adv(v, u, ring, scheme)
        a = dt * a
        return v + a
    for _ in range(nsteps):
        x0 = x
        x = E(x0)
        for c0, c1 in SSP_STAGES[order]:
            x = (c0 * x0) + (c1 * E(x))
        if each is not None:
            each(x)
    return x


def _square(n, dtype):
    x = torch.zeros(n, dtype=dtype)
    x[n // 4:n // 2] = 1.0
    return x


def _tv(x):
    return float((torch.roll(x, -1, 0) - x).abs().to(torch.float64).sum())


SQUARE_RUNS = [(1, 0.25), (1, 0.5), (3, 0.25), (3, 0.5), (3, 0.75)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("lim", LIMITERS)
def test_square_wave_total_variation_and_bounds(lim, dtype):
    n = 64
    eps = torch.finfo(dtype).eps
    for order, cfl in SQUARE_RUNS:
        for u in (1.0, -1.0):
            tvs, lo, hi = [_tv(_square(n, dtype))], [], []

            def each(x):
                tvs.append(_tv(x)); lo.append(float(x.min())); hi.append(float(x.max()))
            ring_march(_square(n, dtype), u, cfl / n, 100, lim, order, each)
            growth = max(b - a for a, b in zip(tvs, tvs[1:]))
            print(f"square {lim} {dtype} order {order} CFL {cfl} u {u}: TV {tvs[0]} -> {tvs[-1]}, max growth per step {growth:.3e}, "
                  f"min {min(lo):.3e}, max - 1 {max(hi) - 1:.3e}")
            assert all(b - a <= 64 * eps * a for a, b in zip(tvs, tvs[1:])), (order, cfl, u, growth)   # ulp of the field's dtype
            assert min(lo) >= 0.0 and max(hi) <= 1.0, (order, cfl, u, min(lo), max(hi))


def test_quick_leaves_the_bounds_on_the_square_wave():
    x = ring_march(_square(64, torch.float64), 1.0, 0.5 / 64, 100, "quick", 3)
    print(f"square quick: min {float(x.min()):.4f}, max {float(x.max()):.4f}")
    assert float(x.min()) < -0.05 and float(x.max()) > 1.05


def test_gaussian_accuracy():
    err = {}
    for scheme in ("upwind", "minmod", "mc"):
        err[scheme] = []
        for n in (64, 128, 256):
            xs = torch.arange(n, dtype=torch.float64) / n
            start = torch.exp(-(((xs - 0.5) / 0.08) ** 2))
            nsteps = int(round(n / 0.4))
            end = ring_march(start, 1.0, 1.0 / nsteps, nsteps, scheme, 3)
            err[scheme].append(float((end - start).abs().sum()) / n)
    print("Gaussian once round, L1 error at 64 / 128 / 256:", err)
    for e in err.values():
        assert e[2] < e[1] < e[0], err
    for i in range(3):
        assert err["mc"][i] < err["minmod"][i] < err["upwind"][i], err


# ---- 6: exact bounds through the march -------------------------------------------------------------------------------
def block_case(dtype):
    """12 x 14 x 16, zero dirichlet walls, the unit block [4:8, 4:9, 5:10], velocity (1, -1, 0.5), dt = 0.45 / sum |u_a| / dx_a"""
    mesh = O.OMesh([0.0] * 3, [1.0] * 3, [12, 14, 16], dtype)
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(3, 0.0, "dirichlet"))
    phi = torch.zeros((1, 12, 14, 16), dtype=mesh.dtype)
    phi[0, 4:8, 4:9, 5:10] = 1.0
    vel = [1.0, -1.0, 0.5]
    dt = 0.45 / sum(abs(v) / h for v, h in zip(vel, mesh.dx_list))
    return mesh, bcs, phi, vel, dt


def rotation_case(dtype):
    """33^2, zero dirichlet walls, the block [8:14, 12:20] in solid-body rotation about the centre, sum-CFL 0.4"""
    mesh = O.OMesh([0.0] * 2, [1.0] * 2, [33, 33], dtype)
    bcs = O.make_bcs(mesh, O.homogeneous_cfg(2, 0.0, "dirichlet"))
    phi = torch.zeros((1, 33, 33), dtype=mesh.dtype)
    phi[0, 8:14, 12:20] = 1.0
    x, y = mesh.grid
    vel = [(-(y - 0.5)).contiguous(), (x - 0.5).contiguous()]
    cfl = (vel[0].abs() / mesh.dx_list[0] + vel[1].abs() / mesh.dx_list[1]).max()
    return mesh, bcs, phi, vel, 0.4 / float(cfl)


@pytest.mark.parametrize("dtype", ["double", "single"])
@pytest.mark.parametrize("lim", LIMITERS)
def test_exact_bounds_through_the_march(lim, dtype):
    for name, case, runs in (("block", block_case, ((1, 60), (3, 40))), ("rotation", rotation_case, ((1, 100), (3, 60)))):
        mesh, bcs, phi, vel, dt = case(dtype)
        for order, nsteps in runs:
            x = phi
            lo, hi = 0.0, 1.0
            for _ in range(nsteps // 10):
                x = Q.march(x, vel, 0.0, dt, 10, mesh, bcs, lim, order)
                lo, hi = min(lo, float(x.min())), max(hi, float(x.max()))
            print(f"{name} {lim} {dtype} order {order}: {nsteps} steps, min {lo:.3e}, max - 1 {hi - 1:.3e}, moved {float((x - phi).abs().max()):.3f}")
            assert lo >= 0.0 and hi <= 1.0, (name, order, lo, hi)
            assert float((x - phi).abs().max()) > 0.3     # it moved


# ---- 8: the checks in front of the device ----------------------------------------------------------------------------
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


@pytest.mark.parametrize("lim", LIMITERS)
def test_explicit_only(lim):
    from pyapes_amd.solver.fdm import FDM
    from pyapes_amd.solver.ops import Solver
    cfg = CONFIG[lim]
    phi = _cpu_field()
    fdm = FDM(cfg)
    solver = Solver({"fdm": {"method": "bicgstab", "tol": 1e-6, "max_it": 10, "report": False}})
    with pytest.raises(NotImplementedError, match=f"{lim} is explicit-only"):
        solver.set_eq(fdm.div(1.0, phi) - fdm.laplacian(0.1, phi) == 0.0)
    with pytest.raises(NotImplementedError, match=f"{lim} is explicit-only"):
        FDC(cfg).div.adjust_rhs(1.0, phi, cfg)
    with pytest.raises(NotImplementedError, match=lim):
        quick_explicit_only(div_kind(lim, False), "here")
    quick_explicit_only(div_kind("upwind", False), "here")
    quick_mesh_check(div_kind(lim, False), phi.mesh, "here")


@pytest.mark.parametrize("lim", LIMITERS)
def test_argument_checks_fire_before_a_device_is_touched(lim, monkeypatch):
    cfg = CONFIG[lim]
    slab = _cpu_field(n=(9, 9, 9), slab=(0, 2))
    cyl = _cpu_field(cyl=True)
    vec = _cpu_field(dim=2)
    phi = _cpu_field()
    real = (M.context_for, M.require_gpu)

    def reached(*a, **k):
        raise AssertionError("a device was touched before the arguments were checked")
    monkeypatch.setattr(M, "context_for", reached)
    monkeypatch.setattr(M, "require_gpu", reached)
    for f in (slab, cyl):
        for call in (lambda: euler_step(f, 1.0, 0.05, 1e-3, cfg), lambda: euler_march(f, 1.0, 0.05, 1e-3, 2, cfg),
                     lambda: FDC(cfg).div(1.0, f)):
            with pytest.raises(NotImplementedError, match=lim):   # the message names the limiter asked for
                call()
        for call in (lambda: rk_step(f, 1.0, 0.05, 1e-3, cfg, order=3), lambda: rk_march(f, 1.0, 0.05, 1e-3, 2, cfg, order=2)):
            with pytest.raises(NotImplementedError):              # (a slab is refused by the Runge-Kutta entries themselves)
                call()
    vslab = _cpu_field(n=(9, 9, 9), dim=3, slab=(0, 2))
    vcyl = _cpu_field(dim=2, cyl=True)
    for f in (vslab, vcyl):
        for call in (lambda: momentum_step(f, 0.05, 1e-3, cfg), lambda: momentum_march(f, 0.05, 1e-3, 2, cfg)):
            with pytest.raises(NotImplementedError):
                call()
    for call in (lambda: rk_march(vec, 1.0, 0.05, 1e-3, 2, cfg), lambda: euler_march(vec, 1.0, 0.05, 1e-3, 2, cfg),
                 lambda: FDC(cfg).div(1.0, vec),                                        # a vector field
                 lambda: FDC({"div": {"limiter": lim, "edge": True}}).div(1.0, phi)):   # edge=True
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match=lim):
        rk_march(phi, 1.0, 0.05, 1e-3, 2, {"div": {"limiter": lim, "compat": True}})
    with pytest.raises(NotImplementedError):   # (the momentum entries refuse compat: True whatever the limiter)
        momentum_march(vec, 0.05, 1e-3, 2, {"div": {"limiter": lim, "compat": True}})
    # past the checks: the operator and the marches need the GPU
    monkeypatch.setattr(M, "context_for", real[0])
    monkeypatch.setattr(M, "require_gpu", real[1])
    _needs_gpu(lambda: FDC(cfg).div(1.0, phi))
    _needs_gpu(lambda: rk_march(phi, 1.0, 0.05, 1e-3, 2, cfg, order=3))
    _needs_gpu(lambda: rk_march(phi, phi, 0.05, 1e-3, 2, cfg, order=3))
    _needs_gpu(lambda: rk_march(phi, (1.0, -1.0), 0.05, 1e-3, 2, cfg, order=3))
    _needs_gpu(lambda: rk_step(phi, 1.0, 0.05, 1e-3, cfg, order=2))
    _needs_gpu(lambda: euler_march(phi, 1.0, 0.05, 1e-3, 2, cfg))
    _needs_gpu(lambda: euler_step(phi, 1.0, 0.05, 1e-3, cfg))
    _needs_gpu(lambda: momentum_march(vec, 0.05, 1e-3, 2, cfg))
    _needs_gpu(lambda: momentum_step(vec, 0.05, 1e-3, cfg))
