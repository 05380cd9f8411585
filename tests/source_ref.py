"""The explicit Euler step with a source term, E_S, the Runge-Kutta stage and the march built from it, restated on the CPU in
torch operation for operation what the device kernels compute (DESIGN.md section 4 "Source term"), from the oracle's own
operators.  Shared by tests/test_source_host.py and tests/test_gpu_source.py.

On the interior set, every operation rounded on its own in the field's dtype:
    a = nu * lap;  a = a - adv;  a = a + s;  a = dt * a;  v = phi + a
s the source at the cell, or the scalar source rounded to the dtype; the ordered BC fill B follows.  Without a source the
``a + s`` operation does not exist, and the result is bit-identical to ``oracle.euler_step`` (tests/test_source_host.py).
A stage is  B(c0 * phi0 + c1 * E_S(phi_s));  S is frozen over a march.  Limiters: "upwind", "none" (central), "quick", "compat" (the literal upwind form).
"""
from __future__ import annotations

from typing import Sequence

import torch
from torch import Tensor

from pyapes_oracle import (apply_div, apply_laplacian, bc_fill, div_tables, div_upwind_intended, interior_slicer,
                           laplacian_tables)
from quick_ref import div_quick

SSP_STAGES = {1: [], 2: [(0.5, 0.5)], 3: [(3.0 / 4.0, 1.0 / 4.0), (1.0 / 3.0, 2.0 / 3.0)]}


def operator_parts(phi: Tensor, u, nu: float, mesh, bcs: Sequence, limiter: str) -> tuple[Tensor, Tensor]:
    """(lap, adv) of the scalar field ``phi`` (1, *n) at every node, as the Euler step reads them"""
    nd = mesh.dim
    lap = apply_laplacian(laplacian_tables(phi, mesh, bcs), phi, nd)
    if limiter == "upwind":
        adv = div_upwind_intended(u, phi, mesh)
    elif limiter == "none":
        adv = apply_div(div_tables(u, phi, mesh, bcs, "none"), phi, nd)
    elif limiter == "compat":   # the reference's literal upwind form (Div limiter "upwind" with compat=True)
        adv = apply_div(div_tables(u, phi, mesh, bcs, "upwind"), phi, nd)
    elif limiter == "quick":
        adv = div_quick(u, phi, mesh, bcs)
    else:
        raise ValueError(limiter)
    return lap, adv


def _source_at(S, phi: Tensor, sl):
    """the operand of ``a + s`` on the interior set: a tensor shaped like ``phi`` or like one component, or a scalar"""
    if isinstance(S, Tensor):
        s = S[0] if S.dim() == phi.dim() else S
        assert s.shape == phi[0].shape and s.dtype == phi.dtype
        return s[sl]
    return float(S)


def euler_step(phi: Tensor, u, nu: float, dt: float, mesh, bcs: Sequence, limiter: str = "upwind", S=None) -> Tensor:
    """E_S: B( phi + dt * ((nu * lap - adv) + s) ) on the interior set"""
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


def rk_stage(phi: Tensor, phi0: Tensor, c0: float, c1: float, u, nu: float, dt: float, mesh, bcs: Sequence,
             limiter: str = "upwind", S=None) -> Tensor:
    e = euler_step(phi, u, nu, dt, mesh, bcs, limiter, S)
    out = (c0 * phi0) + (c1 * e)
    bc_fill(out, bcs)
    return out


def march(phi: Tensor, u, nu: float, dt: float, nsteps: int, mesh, bcs: Sequence, limiter: str = "upwind", order: int = 3,
          S=None, self_adv: bool = False) -> Tensor:
    """``nsteps`` SSP Runge-Kutta steps of ``order`` (1: Euler) with the frozen source S; self_adv: every Euler step / stage is
    advected by its own input"""
    for _ in range(nsteps):
        phi0 = phi
        phi = euler_step(phi0, phi0 if self_adv else u, nu, dt, mesh, bcs, limiter, S)
        for c0, c1 in SSP_STAGES[order]:
            phi = rk_stage(phi, phi0, c0, c1, phi if self_adv else u, nu, dt, mesh, bcs, limiter, S)
    return phi


def fixed_point_source(phi: Tensor, u, nu: float, mesh, bcs: Sequence, limiter: str = "upwind") -> Tensor:
    """S = -(nu * lap - adv) of ``phi`` with the step's own rounded operations, at every node (1, *n): with it ``a + s`` of
    E_S(phi) is an exact zero on the interior set, so a BC-filled ``phi`` is a fixed point of the step, bit for bit"""
    lap, adv = operator_parts(phi, u, nu, mesh, bcs, limiter)
    a = nu * lap
    a = a - adv
    return -a
