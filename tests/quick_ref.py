"""The QUICK advection operator (Div limiter "quick") restated on the CPU in torch, operation for operation what the device
kernels compute (DESIGN.md "QUICK"), built on the oracle's Laplacian, interior set and BC fill.  Shared by
tests/test_quick_host.py and tests/test_gpu_quick.py.

Advective form, the speed taken at the node, u+ = max(u, 0), u- = min(u, 0); per mesh axis a:
    bq = 3/8 (x[+1] + x) - 7/8 x[-1] + 1/8 x[-2]        (with u+)
    fq = 7/8 x[+1] - 3/8 (x[-1] + x) - 1/8 x[+2]        (with u-)
    term_a = (u+ bq + u- fq) * fl(1 / dx_a);   adv = (+0) + term_0 + term_1 + term_2
every operation rounded on its own, in the order of the statements below.  Neighbours wrap around on every axis; on an axis
without a periodic face the half whose far-upwind node would wrap (bq at index <= 1, fq at index >= N - 2) is the central
difference 0.5 (x[+1] - x[-1]) instead.
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import Tensor

from pyapes_oracle import apply_laplacian, bc_fill, interior_slicer, laplacian_tables

SSP_STAGES = {1: [], 2: [(0.5, 0.5)], 3: [(3.0 / 4.0, 1.0 / 4.0), (1.0 / 3.0, 2.0 / 3.0)]}


def _speed(u, var: Tensor) -> Tensor:
    if isinstance(u, Tensor):
        assert u.shape == var.shape, "quick_ref: a speed tensor is field-shaped"
        return u[0]
    return torch.full_like(var[0], float(u))


def div_quick(u, var: Tensor, mesh, bcs: Sequence) -> Tensor:
    """(1, *n): the operator at EVERY node of the scalar field ``var`` (1, *n); ``u`` a float or a field-shaped tensor"""
    assert var.shape[0] == 1
    x = var[0]
    uc = _speed(u, var)
    zeros = torch.zeros_like(x)
    up, um = torch.max(uc, zeros), torch.min(uc, zeros)
    periodic = [False] * mesh.dim
    for bc in bcs or []:
        if bc.type == "periodic":
            periodic[mesh.axis_of(bc.face)] = True
    dx = mesh.dx
    out = torch.zeros_like(x)
    for a in range(mesh.dim):
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
        inv = torch.ones((), dtype=var.dtype) / dx[a]
        p = up * bq
        m = um * fq
        p = p + m
        p = p * inv
        out = out + p
    return out.unsqueeze(0)


def euler_step_quick(phi: Tensor, u, nu: float, dt: float, mesh, bcs: Sequence) -> Tensor:
    """the oracle's euler_step with the QUICK advection term: B( phi + dt (nu lap(phi) - adv(phi)) ) on the interior set"""
    nd = mesh.dim
    S = interior_slicer(nd, bcs)
    lap = apply_laplacian(laplacian_tables(phi, mesh, bcs), phi, nd)
    adv = div_quick(u, phi, mesh, bcs)
    new = phi.clone()
    new[0][S] = phi[0][S] + dt * (nu * lap[0][S] - adv[0][S])
    bc_fill(new, bcs)
    return new


def rk_stage_quick(phi: Tensor, phi0: Tensor, c0: float, c1: float, u, nu: float, dt: float, mesh, bcs: Sequence) -> Tensor:
    e = euler_step_quick(phi, u, nu, dt, mesh, bcs)
    out = (c0 * phi0) + (c1 * e)
    bc_fill(out, bcs)
    return out


def march_quick(phi: Tensor, u, nu: float, dt: float, nsteps: int, mesh, bcs: Sequence, order: int = 3,
                self_adv: bool = False) -> Tensor:
    """``nsteps`` SSP Runge-Kutta steps of ``order``; self_adv: every Euler step / stage is advected by its own input"""
    for _ in range(nsteps):
        phi0 = phi
        phi = euler_step_quick(phi0, phi0 if self_adv else u, nu, dt, mesh, bcs)
        for c0, c1 in SSP_STAGES[order]:
            phi = rk_stage_quick(phi, phi0, c0, c1, phi if self_adv else u, nu, dt, mesh, bcs)
    return phi


def march_limiter(phi: Tensor, u, nu: float, dt: float, nsteps: int, mesh, bcs: Sequence, limiter: str, order: int = 3) -> Tensor:
    """the same march with the oracle's own Euler step (limiter "none" / "upwind"): the schemes QUICK is compared with"""
    import pyapes_oracle as O
    for _ in range(nsteps):
        phi0 = phi
        phi = O.euler_step(phi0, u, nu, dt, mesh, bcs, limiter)
        for c0, c1 in SSP_STAGES[order]:
            e = O.euler_step(phi, u, nu, dt, mesh, bcs, limiter)
            phi = (c0 * phi0) + (c1 * e)
            bc_fill(phi, bcs)
    return phi
