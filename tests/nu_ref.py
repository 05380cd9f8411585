"""The marches with a DIFFUSIVITY FIELD restated on the CPU in torch, on top of tests/march_ref.py and the oracle: the term
div(nu grad phi) with nu per node, and the step, the stage, the march and the momentum march that carry it.  New, defined by this
project (no reference counterpart); operation for operation what the device kernels compute (DESIGN.md section 4 "Diffusivity
field").

Per mesh axis a, every operation rounded on its own in the field's dtype:
    ih = fl(1 / dx_a);  w = ih * ih;  w = 0.5 * w
    nup = nu[+1]_a + nu;  num = nu + nu[-1]_a;  fp = x[+1]_a - x;  fm = x - x[-1]_a
    t = nup * fp;  s = num * fm;  t = t - s;  t = t * w;  d = d + t                  (d starts at +0, axes ascending)
Neighbours wrap around on every axis.  On the interior set
    a = d - adv;  [a = a + s;]  a = dt * a;  v = phi + a
and the ordered BC fill B follows; the advection term, the source, the stage B(c0 phi0 + c1 E(phi_s)) and the rotation of a
march are march_ref's (tvd_ref's for "minmod" / "mc").  The step reads the BC-filled face values of its input, never the Neumann
2/3 rows of the Laplacian tables, and nu at every node the stencil touches: nu has no BCs.  nu is frozen over a march.
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import Tensor

import march_ref as Q
import tvd_ref as TV
from pyapes_oracle import bc_fill, interior_slicer


def component(nu: Tensor, phi: Tensor) -> Tensor:
    """``nu`` -- shaped like ``phi`` (1, *n) or like one component -- as one component"""
    nu = nu[0] if nu.dim() == phi.dim() else nu
    assert nu.shape == phi[0].shape and nu.dtype == phi.dtype
    return nu


def face_weights(x: Tensor, mesh) -> list[Tensor]:
    out = []
    for a in range(mesh.dim):
        ih = torch.ones((), dtype=x.dtype) / mesh.dx[a]
        w = ih * ih
        w = 0.5 * w
        out.append(w)
    return out


def nu_term(phi: Tensor, nu: Tensor, mesh) -> Tensor:
    """(1, *n): d at EVERY node of the scalar field ``phi`` (1, *n)"""
    assert phi.shape[0] == 1
    x, nc = phi[0], component(nu, phi)
    w = face_weights(x, mesh)
    d = torch.zeros_like(x)
    for a in range(mesh.dim):
        nup = torch.roll(nc, -1, a) + nc
        num = nc + torch.roll(nc, 1, a)
        fp = torch.roll(x, -1, a) - x
        fm = x - torch.roll(x, 1, a)
        t = nup * fp
        s = num * fm
        t = t - s
        t = t * w[a]
        d = d + t
    return d.unsqueeze(0)


def advection(phi: Tensor, u, mesh, bcs: Sequence, limiter: str) -> Tensor:
    """(1, *n): the advection term of march_ref / tvd_ref for ``u`` (one speed, or a list / tuple: a velocity)"""
    if limiter in ("minmod", "mc"):
        return TV.adv_tvd(u, phi, mesh, bcs, limiter) if isinstance(u, (list, tuple)) else TV.div_tvd(u, phi, mesh, bcs, limiter)
    return Q.operator_parts(phi, u, 0.0, mesh, bcs, limiter)[1]


def euler_step(phi: Tensor, u, nu: Tensor, dt: float, mesh, bcs: Sequence, limiter: str = "upwind", S=None) -> Tensor:
    """E: B( phi + dt * ((d - adv) [+ s]) ) on the interior set; the signature of march_ref.euler_step, ``nu`` a tensor"""
    assert phi.shape[0] == 1
    sl = interior_slicer(mesh.dim, bcs)
    d = nu_term(phi, nu, mesh)
    adv = advection(phi, u, mesh, bcs, limiter)
    a = d[0][sl] - adv[0][sl]
    if S is not None:
        a = a + Q._source_at(S, phi, sl)
    a = dt * a
    new = phi.clone()
    new[0][sl] = phi[0][sl] + a
    bc_fill(new, bcs)
    return new


def rk_stage(phi: Tensor, phi0: Tensor, c0: float, c1: float, u, nu: Tensor, dt: float, mesh, bcs: Sequence,
             limiter: str = "upwind", S=None) -> Tensor:
    return Q.rk_stage(phi, phi0, c0, c1, u, nu, dt, mesh, bcs, limiter, S, step=euler_step)


def march(phi: Tensor, u, nu: Tensor, dt: float, nsteps: int, mesh, bcs: Sequence, limiter: str = "upwind", order: int = 3,
          S=None, self_adv: bool = False) -> Tensor:
    return Q.march(phi, u, nu, dt, nsteps, mesh, bcs, limiter, order, S, self_adv, step=euler_step)


class momentum:
    """march_ref.momentum with one diffusivity field for every component: a vector field V (d, *n) that advects itself (or is
    advected by the frozen velocity ``u``); ``bcs`` one oracle BC list per component"""

    @staticmethod
    def euler_step(V: Tensor, nu: Tensor, dt: float, mesh, bcs: Sequence[Sequence], limiter: str = "upwind",
                   S: Sequence | None = None, u: Sequence | None = None) -> Tensor:
        vel = Q.momentum._vel(V, u)
        return torch.cat([euler_step(V[c:c + 1], vel, nu, dt, mesh, bcs[c], limiter, None if S is None else S[c])
                          for c in range(V.shape[0])])

    @staticmethod
    def rk_stage(V: Tensor, V0: Tensor, c0: float, c1: float, nu: Tensor, dt: float, mesh, bcs: Sequence[Sequence],
                 limiter: str = "upwind", S: Sequence | None = None, u: Sequence | None = None) -> Tensor:
        vel = Q.momentum._vel(V, u)
        return torch.cat([rk_stage(V[c:c + 1], V0[c:c + 1], c0, c1, vel, nu, dt, mesh, bcs[c], limiter,
                                   None if S is None else S[c]) for c in range(V.shape[0])])

    @staticmethod
    def march(U: Tensor, nu: Tensor, dt: float, nsteps: int, mesh, bcs: Sequence[Sequence], limiter: str = "upwind",
              order: int = 3, S: Sequence | None = None, u: Sequence | None = None) -> Tensor:
        for _ in range(nsteps):
            U0 = U
            U = momentum.euler_step(U0, nu, dt, mesh, bcs, limiter, S, u)
            for c0, c1 in Q.SSP_STAGES[order]:
                U = momentum.rk_stage(U, U0, c0, c1, nu, dt, mesh, bcs, limiter, S, u)
        return U
