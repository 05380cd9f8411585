"""The two projection kernels restated on the CPU in torch, operation for operation what ``k_divergence`` and
``k_project_correct`` compute (include/pyapes_hip.h "projection", DESIGN.md section 4 "Projection"), and the projection step
built from them and the oracle's CG.  A plain module, no test lives here: the yardstick of tests/test_projection_host.py and
tests/test_gpu_projection.py.

Per mesh axis a, every operation rounded on its own in the field's dtype, h_a = 0.5 / dx_a formed in double and converted once
(dx_a the spacing as the mesh dtype stores it), neighbours wrapping around (``torch.roll``):
    divergence   d = U_a[+1]_a - U_a[-1]_a;  d = d * h_a;  s = s + d   (s starts at +0, axes ascending);   out = scale * s
    correction   g = p[+1]_c - p[-1]_c;  g = g * h_c;  g = scale * g;  out_c = U_c - g
on the interior set of the BC list (the oracle's ``interior_slicer``: [1:-1] per axis, an end opened by a periodic face); off
it the divergence is +0 and the correction hands U_c on.  ``scale`` is rounded to the dtype once.  Both read BC-filled inputs:
the caller fills them.
"""
from __future__ import annotations

import warnings
from typing import Sequence

import torch
from torch import Tensor

from pyapes_oracle import bc_fill, interior_slicer, solve_poisson, make_bcs


# ---- the walled single-mode problem (tests/test_projection_host.py derives what the projection leaves of it) ---------------
MODE_N, MODE_M = 17, 4           # the phase advances by theta = MODE_M pi / (MODE_N - 1) = pi / 4 per node on both axes
MODE_DT, MODE_RHO = 0.01, 1.3


def mode_case(dtype: str):
    """(oracle mesh, U, the Dirichlet values of U per face and component): on the unit square, U = (cos sin, 1/2 sin cos) of
    the sine mode sin(theta i) sin(theta j), whose divergence is that mode on the interior set; the faces of U hold the mode's
    own values, p is 0 on every face"""
    import math

    from pyapes_oracle import FACES, OMesh
    om = OMesh([0.0, 0.0], [1.0, 1.0], [MODE_N, MODE_N], dtype)
    th = math.pi * MODE_M / (MODE_N - 1)
    i = torch.arange(MODE_N, dtype=torch.float64)
    I, J = torch.meshgrid(i, i, indexing="ij")
    U = torch.stack([torch.cos(th * I) * torch.sin(th * J), 0.5 * torch.sin(th * I) * torch.cos(th * J)]).to(om.dtype)
    face_vals = [[U[c][om.face_mask(f)].clone() for c in range(2)] for f in FACES[:4]]
    return om, U, face_vals


def inner_norm(d: Tensor) -> float:
    """the 2-norm of a (1, n, n) field over the nodes at least two from a wall"""
    return float(d[0][2:-2, 2:-2].double().norm())


def half_inverse_spacing(mesh, dtype: torch.dtype) -> list[Tensor]:
    """h_a = fl(0.5 / dx_a): the quotient in double, converted to the dtype once"""
    return [torch.tensor(0.5 / float(mesh.dx[a]), dtype=torch.float64).to(dtype) for a in range(mesh.dim)]


def divergence(U: Tensor, mesh, bcs: Sequence, scale: float = 1.0) -> Tensor:
    """(1, *n): ``scale`` times the central divergence of the BC-filled vector ``U`` (d, *n) on the interior set of ``bcs``"""
    assert U.shape[0] == mesh.dim and mesh.dim >= 2
    h = half_inverse_spacing(mesh, U.dtype)
    sc = torch.tensor(float(scale), dtype=torch.float64).to(U.dtype)
    s = torch.zeros_like(U[0])
    for a in range(mesh.dim):
        d = torch.roll(U[a], -1, a) - torch.roll(U[a], 1, a)
        d = d * h[a]
        s = s + d
    sl = interior_slicer(mesh.dim, bcs)
    out = torch.zeros_like(U[0])
    out[sl] = (sc * s)[sl]
    return out.unsqueeze(0)


def correct(U: Tensor, p: Tensor, mesh, bcs: Sequence, scale: float, fill: bool = True) -> Tensor:
    """(d, *n): ``U_c - scale * d_c p`` on the interior set of ``bcs``, U_c off it, then -- ``fill`` -- the ordered BC fill of
    every component (an oracle BC list whose values are lists holds one value per component).  ``p`` (1, *n) BC-filled."""
    assert U.shape[0] == mesh.dim and p.shape[0] == 1
    h = half_inverse_spacing(mesh, U.dtype)
    sc = torch.tensor(float(scale), dtype=torch.float64).to(U.dtype)
    sl = interior_slicer(mesh.dim, bcs)
    out = U.clone()
    for c in range(mesh.dim):
        g = torch.roll(p[0], -1, c) - torch.roll(p[0], 1, c)
        g = g * h[c]
        g = sc * g
        out[c][sl] = (U[c] - g)[sl]
    if fill:
        bc_fill(out, bcs)
    return out


def project(U: Tensor, p: Tensor, dt: float, rho: float, mesh, ubcs: Sequence, pcfg: Sequence[dict], tol: float,
            max_it: int) -> tuple[Tensor, Tensor, dict]:
    """The projection step on the CPU: B(U); -rhs = -(rho / dt) div(U); the oracle's CG on -lap(p) = -rhs with ``p``'s BCs
    (config ``pcfg``) from ``p``'s content; B(p); U <- B(U - (dt / rho) grad(p)).  Returns (U, p, report); the inputs stay."""
    U = bc_fill(U.clone(), ubcs)
    nrhs = divergence(U, mesh, ubcs, -(rho / dt))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, rep = solve_poisson(mesh, pcfg, nrhs, x0=p.clone(), method="cg", tol=tol, max_it=max_it, coeff=1.0, sign=-1.0)
    x = bc_fill(x.clone(), make_bcs(mesh, pcfg))
    return correct(U, x, mesh, ubcs, dt / rho), x, rep
