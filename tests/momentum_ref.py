"""The momentum march -- a vector field U with one component per mesh axis that advects itself,
    dU_c/dt = nu lap(U_c) - (U . grad) U_c + S_c,
restated on the CPU from tests/velocity_ref.py (DESIGN.md section 4 "Momentum").  Shared by tests/test_momentum_host.py and
tests/test_gpu_momentum.py.

Per stage and component c it is ``velocity_ref.euler_step`` / ``rk_stage`` of the scalar V_c with the velocity
u = [V_0, .., V_{d-1}] -- ALL components of the stage's input V, so no component sees another component's output of the same
stage -- and component c's oracle BCs.  ``bcs`` is a list of d oracle BC lists: one BC type per face for all components, the
face values per component.  ``S`` is None or d entries (None, a number or a tensor each); ``u`` a frozen velocity instead of
the input (the linearised form: d scalar marches).
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import Tensor

import velocity_ref as R

SSP_STAGES = R.SSP_STAGES


def _vel(V: Tensor, u: Sequence | None) -> list:
    return [V[a] for a in range(V.shape[0])] if u is None else list(u)


def euler_step(V: Tensor, nu: float, dt: float, mesh, bcs: Sequence[Sequence], limiter: str = "upwind", S: Sequence | None = None,
               u: Sequence | None = None) -> Tensor:
    """E(V): every component stepped from the same input vector"""
    d = V.shape[0]
    assert d == mesh.dim and len(bcs) == d and (S is None or len(S) == d)
    vel = _vel(V, u)
    return torch.cat([R.euler_step(V[c:c + 1], vel, nu, dt, mesh, bcs[c], limiter, None if S is None else S[c]) for c in range(d)])


def rk_stage(V: Tensor, V0: Tensor, c0: float, c1: float, nu: float, dt: float, mesh, bcs: Sequence[Sequence],
             limiter: str = "upwind", S: Sequence | None = None, u: Sequence | None = None) -> Tensor:
    """B_c(c0 V0_c + c1 E(V)_c) for every component"""
    d = V.shape[0]
    vel = _vel(V, u)
    return torch.cat([R.rk_stage(V[c:c + 1], V0[c:c + 1], c0, c1, vel, nu, dt, mesh, bcs[c], limiter, None if S is None else S[c])
                      for c in range(d)])


def march(U: Tensor, nu: float, dt: float, nsteps: int, mesh, bcs: Sequence[Sequence], limiter: str = "upwind", order: int = 3,
          S: Sequence | None = None, u: Sequence | None = None) -> Tensor:
    """``nsteps`` SSP Runge-Kutta steps of ``order``; every stage is advected by ITS OWN input (or by the frozen ``u``)"""
    for _ in range(nsteps):
        U0 = U
        U = euler_step(U0, nu, dt, mesh, bcs, limiter, S, u)
        for c0, c1 in SSP_STAGES[order]:
            U = rk_stage(U, U0, c0, c1, nu, dt, mesh, bcs, limiter, S, u)
    return U
