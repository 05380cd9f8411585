"""The explicit Euler step in a velocity field -- one advection speed per mesh axis -- the Runge-Kutta stage and the march built
from it, restated on the CPU in torch operation for operation what the device kernels compute (DESIGN.md section 4
"Velocity"), from the oracle's own operators and quick_ref.  Shared by tests/test_velocity_host.py and
tests/test_gpu_velocity.py.

``u`` is a list of ``mesh.dim`` entries, each a number (rounded to the field's dtype) or a tensor of one component's shape.
Per active axis a the scheme's own term with that axis's component u_a, every operation rounded on its own:
    upwind   t_a = (max(u_a,0) (x - x[-1]_a) + min(u_a,0) (x[+1]_a - x)) * fl(1/dx_a)
    quick    the bq / fq / fallback halves of quick_ref.div_quick with u_a+ / u_a-
    central  the oracle's div_tables / apply_div on the field stacked mesh.dim times with the velocity as its advection
             tensor: cP = u_a[+1]_a, cC = 0 u_a, cM = -u_a[-1]_a, the periodic-face zeroing, / (2 dx_a)
    adv = (+0) + t_0 + t_1 + ...;   a = nu * lap;  a = a - adv;  [a = a + s;]  a = dt * a;  v = phi + a   on the interior set
then the ordered BC fill B; a stage is B(c0 * phi0 + c1 * E(phi_s)); the velocity (and S) are frozen over a march.
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import Tensor

from pyapes_oracle import apply_div, apply_laplacian, bc_fill, div_tables, interior_slicer, laplacian_tables

SSP_STAGES = {1: [], 2: [(0.5, 0.5)], 3: [(3.0 / 4.0, 1.0 / 4.0), (1.0 / 3.0, 2.0 / 3.0)]}


def components(u: Sequence, phi: Tensor) -> list[Tensor]:
    """the velocity as one tensor of a component's shape per mesh axis (a number: filled, i.e. rounded to the dtype)"""
    nd = phi.dim() - 1
    assert len(u) == nd, "velocity_ref: one entry per mesh axis"
    out = []
    for e in u:
        if isinstance(e, Tensor):
            assert e.shape == phi[0].shape and e.dtype == phi.dtype
            out.append(e)
        else:
            out.append(torch.full_like(phi[0], float(e)))
    return out


def adv_upwind(u: Sequence, phi: Tensor, mesh) -> Tensor:
    x = phi[0]
    zeros = torch.zeros_like(x)
    out = torch.zeros_like(x)
    for a, ua in enumerate(components(u, phi)):
        up, um = torch.max(ua, zeros), torch.min(ua, zeros)
        inv = torch.ones((), dtype=phi.dtype) / mesh.dx[a]
        bwd = x - torch.roll(x, 1, a)
        fwd = torch.roll(x, -1, a) - x
        t = up * bwd
        m = um * fwd
        t = t + m
        t = t * inv
        out = out + t
    return out.unsqueeze(0)


def adv_quick(u: Sequence, phi: Tensor, mesh, bcs: Sequence) -> Tensor:
    x = phi[0]
    zeros = torch.zeros_like(x)
    periodic = [False] * mesh.dim
    for bc in bcs or []:
        if bc.type == "periodic":
            periodic[mesh.axis_of(bc.face)] = True
    out = torch.zeros_like(x)
    for a, ua in enumerate(components(u, phi)):
        up, um = torch.max(ua, zeros), torch.min(ua, zeros)
        n = x.shape[a]
        assert n >= 5, "quick: an axis needs at least 5 nodes"
        xp, xm = torch.roll(x, -1, a), torch.roll(x, 1, a)
        xpp, xmm = torch.roll(x, -2, a), torch.roll(x, 2, a)
        t = xp + x
        t = 0.375 * t
        s = 0.875 * xm
        t = t - s
        s = 0.125 * xmm
        bq = t + s
        t = xm + x
        t = 0.375 * t
        s = 0.875 * xp
        t = s - t
        s = 0.125 * xpp
        fq = t - s
        if not periodic[a]:
            cen = xp - xm
            cen = 0.5 * cen
            idx = torch.arange(n).reshape([n if q == a else 1 for q in range(mesh.dim)])
            bq = torch.where(idx <= 1, cen, bq)
            fq = torch.where(idx >= n - 2, cen, fq)
        inv = torch.ones((), dtype=phi.dtype) / mesh.dx[a]
        p = up * bq
        m = um * fq
        p = p + m
        p = p * inv
        out = out + p
    return out.unsqueeze(0)


def adv_central(u: Sequence, phi: Tensor, mesh, bcs: Sequence) -> Tensor:
    nd = mesh.dim
    stacked = phi[0].unsqueeze(0).repeat(nd, *([1] * nd))
    vel = torch.stack(components(u, phi))
    return apply_div(div_tables(vel, stacked, mesh, bcs, "none"), stacked, nd)


def operator_parts(phi: Tensor, u: Sequence, nu: float, mesh, bcs: Sequence, limiter: str) -> tuple[Tensor, Tensor]:
    """(lap, adv) of the scalar field ``phi`` (1, *n) at every node, as the Euler step reads them"""
    lap = apply_laplacian(laplacian_tables(phi, mesh, bcs), phi, mesh.dim)
    if limiter == "upwind":
        adv = adv_upwind(u, phi, mesh)
    elif limiter == "none":
        adv = adv_central(u, phi, mesh, bcs)
    elif limiter == "quick":
        adv = adv_quick(u, phi, mesh, bcs)
    else:
        raise ValueError(limiter)
    return lap, adv


def _source_at(S, phi: Tensor, sl):
    if isinstance(S, Tensor):
        s = S[0] if S.dim() == phi.dim() else S
        assert s.shape == phi[0].shape and s.dtype == phi.dtype
        return s[sl]
    return float(S)


def euler_step(phi: Tensor, u: Sequence, nu: float, dt: float, mesh, bcs: Sequence, limiter: str = "upwind", S=None) -> Tensor:
    """B( phi + dt * ((nu * lap - adv) [+ s]) ) on the interior set, adv formed with one speed per axis"""
    assert phi.shape[0] == 1
    sl = interior_slicer(mesh.dim, bcs)
    lap, adv = operator_parts(phi, u, nu, mesh, bcs, limiter)
    a = nu * lap[0][sl]
    a = a - adv[0][sl]
    if S is not None:
        a = a + _source_at(S, phi, sl)
    a = dt * a
    new = phi.clone()
    new[0][sl] = phi[0][sl] + a
    bc_fill(new, bcs)
    return new


def rk_stage(phi: Tensor, phi0: Tensor, c0: float, c1: float, u: Sequence, nu: float, dt: float, mesh, bcs: Sequence,
             limiter: str = "upwind", S=None) -> Tensor:
    e = euler_step(phi, u, nu, dt, mesh, bcs, limiter, S)
    out = (c0 * phi0) + (c1 * e)
    bc_fill(out, bcs)
    return out


def march(phi: Tensor, u: Sequence, nu: float, dt: float, nsteps: int, mesh, bcs: Sequence, limiter: str = "upwind",
          order: int = 3, S=None) -> Tensor:
    """``nsteps`` SSP Runge-Kutta steps of ``order`` (1: Euler) in the frozen velocity ``u`` (and with the frozen source S)"""
    for _ in range(nsteps):
        phi0 = phi
        phi = euler_step(phi0, u, nu, dt, mesh, bcs, limiter, S)
        for c0, c1 in SSP_STAGES[order]:
            phi = rk_stage(phi, phi0, c0, c1, u, nu, dt, mesh, bcs, limiter, S)
    return phi
