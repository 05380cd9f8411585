"""The slope-limited (TVD) advection schemes, Div limiters "minmod" and "mc" (PA_OP_DIV_MINMOD = 6, PA_OP_DIV_MC = 7), restated
on the CPU in torch, operation for operation what the device kernels compute (include/pyapes_hip.h, DESIGN.md section 4
"Bounded advection").  Built on the pieces of tests/march_ref.py -- the velocity components, the Laplacian half, the source
operand, the stage combination and the march rotation -- with the advection term of this file in the Euler step.

Advective form, the speed taken at the node, u+ = max(u, 0), u- = min(u, 0); per mesh axis a, neighbours wrapping around,
every operation rounded on its own in the field's dtype:
    dm = x - x[-1];  dp = x[+1] - x;  dmm = x[-1] - x[-2];  dpp = x[+2] - x[+1]
    s0 = L(dm, dp);  sm = L(dmm, dm);  sp = L(dp, dpp)
    t = s0 - sm;  t = 0.5 t;  bq = dm + t            (with u+)
    t = sp - s0;  t = 0.5 t;  fq = dp - t            (with u-)
    p = u+ bq;  m = u- fq;  p = p + m;  term_a = p * fl(1 / dx_a);      adv = (+0) + term_0 + term_1 + term_2
L = minmod:  v = 0;  a, b >= 0: the smaller;  a, b < 0: the larger;  a * b <= 0: 0.     L = mc:  v = minmod(a, b); s = a + b;
minmod(2 v, s / 2).  On an axis without a periodic face the half whose far-upwind node would wrap is first-order upwind:
bq = dm at index <= 1, fq = dp at index >= N - 2.
"""
from __future__ import annotations

from typing import Callable, Sequence

import torch
from torch import Tensor

import march_ref as Q
from pyapes_oracle import apply_laplacian, bc_fill, interior_slicer, laplacian_tables


def minmod(a: Tensor, b: Tensor) -> Tensor:
    """minmod1 of csrc/pa_rfp.hip, statement for statement"""
    zero = torch.zeros_like(a)
    v = zero
    v = torch.where((a >= 0) & (b >= 0), torch.where(a < b, a, b), v)
    v = torch.where((a < 0) & (b < 0), torch.where(a > b, a, b), v)
    v = torch.where(a * b <= 0, zero, v)
    return v


def mc(a: Tensor, b: Tensor) -> Tensor:
    """k_limiter's monotonized central: v = minmod(a, b); s = a + b; minmod(2 v, s / 2)"""
    v = minmod(a, b)
    s = a + b
    return minmod(2 * v, s / 2)


def no_slope(a: Tensor, b: Tensor) -> Tensor:
    """L == 0: the scheme is first-order upwind (tests/test_tvd_host.py)"""
    return torch.zeros_like(a)


LIMITERS: dict[str, Callable[[Tensor, Tensor], Tensor]] = {"minmod": minmod, "mc": mc}


def _slope(limiter) -> Callable[[Tensor, Tensor], Tensor]:
    return limiter if callable(limiter) else LIMITERS[limiter]


def tvd_halves(x: Tensor, a: int, periodic: bool, limiter) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(bq, fq, dm, dp) of the component ``x`` (*n) along mesh axis ``a``"""
    L = _slope(limiter)
    n = x.shape[a]
    assert n >= 5, "minmod / mc: an axis needs at least 5 nodes"
    xp, xm = torch.roll(x, -1, a), torch.roll(x, 1, a)
    xpp, xmm = torch.roll(x, -2, a), torch.roll(x, 2, a)
    dm = x - xm
    dp = xp - x
    dmm = xm - xmm
    dpp = xpp - xp
    s0 = L(dm, dp)
    sm = L(dmm, dm)
    sp = L(dp, dpp)
    t = s0 - sm
    t = 0.5 * t
    bq = dm + t
    t = sp - s0
    t = 0.5 * t
    fq = dp - t
    if not periodic:
        idx = torch.arange(n).reshape([n if q == a else 1 for q in range(x.dim())])
        bq = torch.where(idx <= 1, dm, bq)
        fq = torch.where(idx >= n - 2, dp, fq)
    return bq, fq, dm, dp


def tvd_term(x: Tensor, up: Tensor, um: Tensor, a: int, periodic: bool, mesh, limiter) -> Tensor:
    """term_a with the speed halves ``up`` / ``um``"""
    bq, fq, _, _ = tvd_halves(x, a, periodic, limiter)
    inv = torch.ones((), dtype=x.dtype) / mesh.dx[a]
    p = up * bq
    m = um * fq
    p = p + m
    p = p * inv
    return p


def div_tvd(u, var: Tensor, mesh, bcs: Sequence, limiter) -> Tensor:
    """(1, *n): the operator at EVERY node of the scalar field ``var`` (1, *n); ``u`` a float or a field-shaped tensor"""
    assert var.shape[0] == 1
    x = var[0]
    if isinstance(u, Tensor):
        assert u.shape == var.shape, "div_tvd: a speed tensor is field-shaped"
        uc = u[0]
    else:
        uc = torch.full_like(x, float(u))
    zeros = torch.zeros_like(x)
    up, um = torch.max(uc, zeros), torch.min(uc, zeros)
    periodic = Q._periodic_axes(mesh, bcs)
    out = torch.zeros_like(x)
    for a in range(mesh.dim):
        out = out + tvd_term(x, up, um, a, periodic[a], mesh, limiter)
    return out.unsqueeze(0)


def adv_tvd(u: Sequence, phi: Tensor, mesh, bcs: Sequence, limiter) -> Tensor:
    """a velocity: one speed per mesh axis (march_ref.components)"""
    x = phi[0]
    zeros = torch.zeros_like(x)
    periodic = Q._periodic_axes(mesh, bcs)
    out = torch.zeros_like(x)
    for a, ua in enumerate(Q.components(u, phi)):
        up, um = torch.max(ua, zeros), torch.min(ua, zeros)
        out = out + tvd_term(x, up, um, a, periodic[a], mesh, limiter)
    return out.unsqueeze(0)


def euler_step(phi: Tensor, u, nu: float, dt: float, mesh, bcs: Sequence, limiter="minmod", S=None) -> Tensor:
    """march_ref.euler_step with the limited advection term: B( phi + dt * ((nu * lap - adv) [+ s]) ) on the interior set"""
    assert phi.shape[0] == 1
    sl = interior_slicer(mesh.dim, bcs)
    lap = apply_laplacian(laplacian_tables(phi, mesh, bcs), phi, mesh.dim)
    adv = adv_tvd(u, phi, mesh, bcs, limiter) if isinstance(u, (list, tuple)) else div_tvd(u, phi, mesh, bcs, limiter)
    a = nu * lap[0][sl]
    a = a - adv[0][sl]
    if S is not None:
        a = a + Q._source_at(S, phi, sl)
    a = dt * a
    new = phi.clone()
    new[0][sl] = phi[0][sl] + a
    bc_fill(new, bcs)
    return new


def rk_stage(phi: Tensor, phi0: Tensor, c0: float, c1: float, u, nu: float, dt: float, mesh, bcs: Sequence, limiter="minmod",
             S=None) -> Tensor:
    return Q.rk_stage(phi, phi0, c0, c1, u, nu, dt, mesh, bcs, limiter, S, step=euler_step)


def march(phi: Tensor, u, nu: float, dt: float, nsteps: int, mesh, bcs: Sequence, limiter="minmod", order: int = 3, S=None,
          self_adv: bool = False) -> Tensor:
    return Q.march(phi, u, nu, dt, nsteps, mesh, bcs, limiter, order, S, self_adv, step=euler_step)


class momentum:
    """march_ref.momentum with the limited advection term: a vector field V (d, *n) that advects itself (or is advected by the
    frozen velocity ``u``); ``bcs`` one oracle BC list per component"""

    @staticmethod
    def euler_step(V: Tensor, nu: float, dt: float, mesh, bcs: Sequence[Sequence], limiter="minmod", S: Sequence | None = None,
                   u: Sequence | None = None) -> Tensor:
        d = V.shape[0]
        assert d == mesh.dim and len(bcs) == d and (S is None or len(S) == d)
        vel = Q.momentum._vel(V, u)
        return torch.cat([euler_step(V[c:c + 1], vel, nu, dt, mesh, bcs[c], limiter, None if S is None else S[c])
                          for c in range(d)])

    @staticmethod
    def rk_stage(V: Tensor, V0: Tensor, c0: float, c1: float, nu: float, dt: float, mesh, bcs: Sequence[Sequence],
                 limiter="minmod", S: Sequence | None = None, u: Sequence | None = None) -> Tensor:
        vel = Q.momentum._vel(V, u)
        return torch.cat([rk_stage(V[c:c + 1], V0[c:c + 1], c0, c1, vel, nu, dt, mesh, bcs[c], limiter,
                                   None if S is None else S[c]) for c in range(V.shape[0])])

    @staticmethod
    def march(U: Tensor, nu: float, dt: float, nsteps: int, mesh, bcs: Sequence[Sequence], limiter="minmod", order: int = 3,
              S: Sequence | None = None, u: Sequence | None = None) -> Tensor:
        for _ in range(nsteps):
            U0 = U
            U = momentum.euler_step(U0, nu, dt, mesh, bcs, limiter, S, u)
            for c0, c1 in Q.SSP_STAGES[order]:
                U = momentum.rk_stage(U, U0, c0, c1, nu, dt, mesh, bcs, limiter, S, u)
        return U
