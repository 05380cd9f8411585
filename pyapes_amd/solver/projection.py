"""Pressure projection of a collocated velocity field (new; the reference has no counterpart): the step that follows the
momentum predictor ``momentum_step`` in Chorin's non-incremental splitting of the incompressible Navier-Stokes equations,

    U*  = momentum_step(U)                      dU/dt = nu lap(U) - (U . grad) U + S
    lap(p) = (rho / dt) div(U*)                 the existing ``Solver`` on the scalar Field ``p``, ``p``'s own BCs
    U   = B( U* - (dt / rho) grad(p) )          every component's BC fill with its own face values

``divergence(U, scale, out)``: ``scale`` times the central divergence of the BC-filled vector Field ``U`` on the interior set,
+0 off it, in ONE pass over the components (``pa_divergence``: d + 1 arrays moved, where ``mesh.dim`` calls of ``fdm.grad`` and
the sums behind them move about four times as many).  Per mesh axis a, every operation rounded on its own in the mesh dtype,
h_a = 0.5 / dx_a formed in double and converted once:

    d = U_a[+1]_a - U_a[-1]_a;  d = d * h_a;  s = s + d      (s starts at +0, axes ascending);      out = scale * s

``project(U, p, dt, rho, solver)``: the three statements above -- the right-hand side, the solve for ``p`` from ``p``'s current
content, ``p.apply_bcs()``, and the correction  g = p[+1]_c - p[-1]_c; g = g * h_c; g = (dt / rho) * g; U_c = U_c - g  of every
component in one launch (``pa_project_correct``), in place, followed by the ordered BC fill of every component.

``ns_step(U, p, nu, dt, ...)``: ``momentum_step`` followed by ``project``; ``U``'s time advances by ``dt``.

This is an APPROXIMATE projection.  The central divergence and the central gradient compose to the WIDE Laplacian
(p[+2] - 2 p + p[-2]) / (2 h)^2, while the solvers invert the compact one, (p[+1] - 2 p + p[-1]) / h^2.  For a Fourier mode of
wavenumber k the two symbols are sin^2(k h) / h^2 and 4 sin^2(k h / 2) / h^2, so the projection removes the fraction
cos^2(k h / 2) of the mode's divergence and leaves sin^2(k h / 2) of it: the remaining discrete divergence is O(h^2) of the
original, not rounding.  An exact discrete projection needs the wide Laplacian (which decouples odd and even nodes) or a
staggered grid; neither is built.  Not built either: the incremental (pressure-carrying) form, slab and axisymmetric meshes.
"""
from __future__ import annotations

from typing import Any

import torch
from torch import Tensor

from ..backend import require_gpu
from ..hip.context import context_for
from ..variables import Field
from .fdm import FDM
from .march import momentum_step
from .ops import Solver

# the default solve of ``project``: CG on  -lap(p) = -rhs
DEFAULT_SOLVER: dict[str, dict[str, Any]] = {"fdm": {"method": "cg", "tol": 1e-6, "max_it": 1000, "report": False}}


def _vector_args(U: Any, what: str) -> None:
    """the checks of the velocity, made before a device is touched"""
    if not isinstance(U, Field):
        raise TypeError(f"pyapes_amd: {what}: U is a vector Field (got {type(U).__name__})")
    mesh = U.mesh
    if getattr(mesh, "slab", None) is not None:
        raise NotImplementedError(f"pyapes_amd: {what} on a slab mesh (single GPU only)")
    if mesh.coord_sys == "rz":
        raise NotImplementedError(f"pyapes_amd: {what} on an axisymmetric (rz) mesh")
    if mesh.dim < 2:
        raise NotImplementedError(f"pyapes_amd: {what}: a 1-D mesh (a vector field with one component per mesh axis, 2-D or 3-D)")
    if U.dim != mesh.dim:
        raise NotImplementedError(f"pyapes_amd: {what}: a vector field with one component per mesh axis ({U.dim} for {mesh.dim})")


def _project_args(U: Any, p: Any, dt: Any, rho: Any, what: str) -> None:
    """every check of ``project`` / ``ns_step``, made before a device is touched"""
    _vector_args(U, what)
    if not isinstance(p, Field) or p.dim != 1:
        raise TypeError(f"pyapes_amd: {what}: p is a scalar Field (got {type(p).__name__}"
                        + (f" with {p.dim} components)" if isinstance(p, Field) else ")"))
    if p.mesh is not U.mesh:
        raise ValueError(f"pyapes_amd: {what}: the pressure Field lives on another mesh")
    if p().dtype != U().dtype:
        raise ValueError(f"pyapes_amd: {what}: p dtype {p().dtype} != U dtype {U().dtype}")
    if p().device != U().device:
        raise ValueError(f"pyapes_amd: {what}: p on {p().device}, U on {U().device}")
    for name, v in (("dt", dt), ("rho", rho)):
        if isinstance(v, bool) or not isinstance(v, (float, int)):
            raise TypeError(f"pyapes_amd: {what}: {name} is a number (got {type(v).__name__})")
        if not v > 0:
            raise ValueError(f"pyapes_amd: {what}: {name} = {v!r} (a positive number)")


def _divergence(U: Field, scale: float, out: Tensor | None, what: str) -> Tensor:
    require_gpu(U(), what)
    if not U().is_contiguous():
        U.set_var_tensor(U().contiguous())
    U.apply_bcs()
    comp = tuple(U().shape[1:])
    if out is None:
        out = torch.empty((1, *comp), dtype=U().dtype, device=U().device)
    context_for(U.mesh).divergence(U(), scale, out[0] if out.dim() == len(comp) + 1 else out)
    return out


def divergence(U: Field, scale: float = 1.0, out: Tensor | None = None) -> Tensor:
    """``scale * div(U)`` of the vector Field ``U`` (``U.dim == mesh.dim >= 2``) on the interior set, +0 off it: a ``(1, *n)``
    tensor (``out``, shaped like it or like one component, is filled and returned when given).  ``U.apply_bcs()`` runs first:
    the stencil reads the BC-filled face values.  One kernel, ``pa_divergence`` (module docstring)."""
    _vector_args(U, "divergence")
    if isinstance(scale, bool) or not isinstance(scale, (float, int)):
        raise TypeError(f"pyapes_amd: divergence: scale is a number (got {type(scale).__name__})")
    if out is not None:
        comp = tuple(U().shape[1:])
        if not isinstance(out, Tensor) or tuple(out.shape) not in ((1, *comp), comp):
            raise ValueError(f"pyapes_amd: divergence: out is a Tensor of shape {(1, *comp)} or {comp}")
        if out.dtype != U().dtype:
            raise ValueError(f"pyapes_amd: divergence: out dtype {out.dtype} != mesh dtype {U().dtype}")
        if out.device != U().device:
            raise ValueError(f"pyapes_amd: divergence: out on {out.device}, the field on {U().device}")
    return _divergence(U, float(scale), out, "divergence")


def project(U: Field, p: Field, dt: float, rho: float = 1.0, solver: dict | None = None) -> dict:
    """Make ``U`` (approximately, module docstring) divergence-free: solve ``lap(p) = (rho / dt) div(U)`` for the scalar Field
    ``p`` -- with ``p``'s own BCs, from ``p``'s current content -- and correct ``U <- B(U - (dt / rho) grad(p))`` in place.
    ``solver``: the ``{"fdm": {...}}`` dict a ``Solver`` takes (default: CG, tol 1e-6, at most 1000 iterations); the equation
    is handed over as ``-laplacian(1.0, p) == -rhs``, the form that is positive definite.  Returns the solver's report.
    Nothing is allocated per call beyond the right-hand side."""
    _project_args(U, p, dt, rho, "project")
    return _project(U, p, float(dt), float(rho), solver, "project")


def _project(U: Field, p: Field, dt: float, rho: float, solver: dict | None, what: str) -> dict:
    # -rhs, formed by the kernel itself: (-s) * x and -(s * x) are the same bits
    nrhs = _divergence(U, -(rho / dt), None, what)
    sol = Solver(DEFAULT_SOLVER if solver is None else solver)
    sol.set_eq(-FDM().laplacian(1.0, p) == nrhs)
    report = sol.solve()
    p.apply_bcs()
    ctx = context_for(U.mesh)
    ctx.bind_bcs(U(), U.bcs, 0)
    ctx.project_correct(U(), p()[0], dt / rho, U.bcs)
    return report


def ns_step(U: Field, p: Field, nu: float | Tensor | Field, dt: float, config: dict | None = None, order: int = 3, *,
            rho: float = 1.0, source: Tensor | Field | tuple | list | None = None, solver: dict | None = None) -> dict:
    """One step of the incompressible Navier-Stokes equations in Chorin's non-incremental form: ``momentum_step(U, nu, dt,
    config, order, source=source)``, then ``project(U, p, dt, rho, solver)``.  ``U``'s time advances by ``dt``; returns the
    solver's report.  Every check of both halves is made before a device is touched."""
    _project_args(U, p, dt, rho, "ns_step")
    momentum_step(U, nu, dt, config, order, source=source)
    report = _project(U, p, float(dt), float(rho), solver, "ns_step")
    if hasattr(U, "_t"):
        U.update_time(dt)
    return report
