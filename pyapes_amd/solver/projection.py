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
staggered grid; neither is built.  Not built either: slab and axisymmetric meshes.

``form=`` on ``project`` / ``ns_step``: ``"chorin"`` (the default) is the splitting above.  ``"incremental"`` and ``"rotational"``
CARRY the pressure: the predictor feels ``-grad(p^n) / rho`` and the solve is for the increment ``phi``, which is O(dt) of ``p``.
One step is these statements in this order, every operation rounded on its own in the mesh dtype, the scalars 1 / rho,
dt / rho, -(rho / dt) and nu dt formed in double and converted once:

    1  B(p)
    2  src_c = S_c - (1 / rho) grad_c(p)  on the interior set, S_c off it   (``pa_project_correct``, out of place, no fill;
                                                                            S: ``source`` as a (d, *n) tensor, zeros for None)
    3  momentum_step(U, nu, dt, config, order, source=src)
    4  nrhs = -(rho / dt) div(U)                                            (``divergence``)
    5  phi = +0;  solve  -lap(phi) = nrhs  with phi's BCs -- the homogeneous counterparts of p's;  B(phi)
    6  U_c <- U_c - (dt / rho) grad_c(phi)  on the interior set;  p <- p + phi  at every node;
       "rotational":  t = (nu dt) nrhs;  p <- p + t   (p + phi - nu rho div(U*));  then B(U)          (``pa_project_update``)
    7  B(p);  U's time advances by dt

A fluid at rest under a body force f = grad(p0) / rho with p = p0 is a FIXED POINT of these statements, bit for bit: statement 2
gives an exact zero, U stays +0, nrhs is a zero, the solve returns after one iteration with phi = +0, and p keeps its bits.
Chorin's form accelerates that fluid by dt f and cannot restore the balance with the approximate projection (DESIGN.md section 4
"Incremental form" has the figures).  ``project(..., form=)`` is statements 4 - 7 with ``p`` read as p^n.

``flow_stats(U, dt)``: the CFL rate max sum_a |U_a| / dx_a, the divergence that is left (its maximum and its sum of squares on the
interior set) and the sum of squares of U, in ONE pass (``pa_flow_stats``).  ``ns_march``: a loop of ``ns_step`` with an optional
CFL cap on every step's dt.
"""
from __future__ import annotations

from typing import Any

import math

import torch
from torch import Tensor

from ..backend import require_gpu
from ..hip.context import context_for
from ..variables import Field
from .fdm import FDM
from .march import _Component, _diffusivity_of, _momentum_args, momentum_step
from .ops import Solver

# the default solve of ``project``: CG on  -lap(p) = -rhs
DEFAULT_SOLVER: dict[str, dict[str, Any]] = {"fdm": {"method": "cg", "tol": 1e-6, "max_it": 1000, "report": False}}
FORMS = ("chorin", "incremental", "rotational")


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


def _number(name: str, v: Any, what: str, positive: bool = True, optional: bool = False) -> None:
    """``v`` is a number, not a bool (``optional``: or None), and -- ``positive`` -- > 0, which refuses NaN"""
    if v is None and optional:
        return
    if isinstance(v, bool) or not isinstance(v, (float, int)):
        raise TypeError(f"pyapes_amd: {what}: {name} is a number{' or None' if optional else ''} (got {type(v).__name__})")
    if positive and not v > 0:
        raise ValueError(f"pyapes_amd: {what}: {name} = {v!r} (a positive number)")


_SCALAR_FIELDS = {"p": "pressure Field", "phi": "increment Field phi"}


def _scalar_field(name: str, f: Any, U: Field, what: str) -> None:
    """``f`` (``p`` or ``phi``) is a scalar Field on ``U``'s mesh, of ``U``'s dtype and device"""
    if not isinstance(f, Field) or f.dim != 1:
        raise TypeError(f"pyapes_amd: {what}: {name} is a scalar Field (got {type(f).__name__}"
                        + (f" with {f.dim} components)" if isinstance(f, Field) else ")"))
    if f.mesh is not U.mesh:
        raise ValueError(f"pyapes_amd: {what}: the {_SCALAR_FIELDS[name]} lives on another mesh")
    if f().dtype != U().dtype:
        raise ValueError(f"pyapes_amd: {what}: {name} dtype {f().dtype} != U dtype {U().dtype}")
    if f().device != U().device:
        raise ValueError(f"pyapes_amd: {what}: {name} on {f().device}, U on {U().device}")


def _project_args(U: Any, p: Any, dt: Any, rho: Any, form: Any, phi: Any, nu: Any, what: str) -> None:
    """every check of ``project`` / ``ns_step`` / ``ns_march`` on the velocity, the pressure, the numbers and ``form=`` /
    ``phi=``, made before a device is touched"""
    _vector_args(U, what)
    _scalar_field("p", p, U, what)
    _number("dt", dt, what)
    _number("rho", rho, what)
    if not isinstance(form, str) or form not in FORMS:
        raise ValueError(f"pyapes_amd: {what}: form {form!r} (one of {', '.join(FORMS)})")
    if form == "rotational":
        if isinstance(nu, (Tensor, Field)):
            raise NotImplementedError(f"pyapes_amd: {what}: form 'rotational' with a diffusivity field (the term nu rho div(U*) "
                                      "is defined for a number)")
        if isinstance(nu, bool) or not isinstance(nu, (float, int)):
            raise TypeError(f"pyapes_amd: {what}: form 'rotational' needs nu, a number (got {type(nu).__name__})")
    if phi is not None:
        if phi is p:
            raise ValueError(f"pyapes_amd: {what}: phi is p itself (the increment needs a Field of its own)")
        _scalar_field("phi", phi, U, what)


def _increment_of(p: Field, phi: Field | None) -> Field:
    """the Field that receives the increment: the caller's, or one built once from ``p``'s BC config with every value
    replaced by 0.0 (the homogeneous counterpart; a face without a value -- periodic -- keeps None) and kept on ``p``"""
    if phi is not None:
        return phi
    phi = getattr(p, "_increment", None)
    if phi is None or phi.mesh is not p.mesh or phi().dtype != p().dtype or phi().device != p().device:
        dom = [dict(bc, bc_val=None if bc["bc_val"] is None else 0.0) for bc in p.bc_config["domain"]]
        phi = Field(p.name + "_increment", 1, p.mesh, {"domain": dom, "obstacle": None})
        p._increment = phi
    return phi


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
    _number("scale", scale, "divergence", positive=False)
    if out is not None:
        comp = tuple(U().shape[1:])
        if not isinstance(out, Tensor) or tuple(out.shape) not in ((1, *comp), comp):
            raise ValueError(f"pyapes_amd: divergence: out is a Tensor of shape {(1, *comp)} or {comp}")
        if out.dtype != U().dtype:
            raise ValueError(f"pyapes_amd: divergence: out dtype {out.dtype} != mesh dtype {U().dtype}")
        if out.device != U().device:
            raise ValueError(f"pyapes_amd: divergence: out on {out.device}, the field on {U().device}")
    return _divergence(U, float(scale), out, "divergence")


def project(U: Field, p: Field, dt: float, rho: float = 1.0, solver: dict | None = None, form: str = "chorin",
            phi: Field | None = None, nu: float | None = None) -> dict:
    """Make ``U`` (approximately, module docstring) divergence-free: solve ``lap(p) = (rho / dt) div(U)`` for the scalar Field
    ``p`` -- with ``p``'s own BCs, from ``p``'s current content -- and correct ``U <- B(U - (dt / rho) grad(p))`` in place.
    ``solver``: the ``{"fdm": {...}}`` dict a ``Solver`` takes (default: CG, tol 1e-6, at most 1000 iterations); the equation
    is handed over as ``-laplacian(1.0, p) == -rhs``, the form that is positive definite.  Returns the solver's report.
    Nothing is allocated per call beyond the right-hand side.

    ``form`` "incremental" / "rotational" (module docstring, statements 4 - 7): ``p`` is read as p^n and UPDATED by the
    increment, which is solved for from zero in ``phi`` (a scalar Field with the homogeneous counterparts of ``p``'s BCs; None:
    built once and kept on ``p``).  "rotational" needs ``nu``, a number.  ``phi`` and ``nu`` are not read by "chorin"."""
    _project_args(U, p, dt, rho, form, phi, nu, "project")
    return _project(U, p, float(dt), float(rho), solver, form, phi, nu, "project")


def _project(U: Field, p: Field, dt: float, rho: float, solver: dict | None, form: str, phi: Field | None, nu: float | None,
             what: str) -> dict:
    """statements 4 - 7 of the module docstring but the time stamp.  "chorin" is the same sequence with ``p`` itself solved
    for, from its current content, a right-hand side of its own, and the plain correction at the end"""
    carried = form != "chorin"
    x, out = p, None                                         # the Field that is solved for; where the right-hand side goes
    if carried:
        require_gpu(U(), what)
        out = context_for(U.mesh).work("projection nrhs", 1)
        x = _increment_of(p, phi)
    # -rhs, formed by the kernel itself: (-s) * x and -(s * x) are the same bits
    nrhs = _divergence(U, -(rho / dt), out, what)
    if carried:
        if not x().is_contiguous():
            x.set_var_tensor(torch.empty_like(p()))
        x().zero_()                                          # no state between calls: a step on a used mesh is a fresh one
    sol = Solver(DEFAULT_SOLVER if solver is None else solver)
    sol.set_eq(-FDM().laplacian(1.0, x) == nrhs)
    report = sol.solve()
    x.apply_bcs()
    if carried and not p().is_contiguous():
        p.set_var_tensor(p().contiguous())
    ctx = context_for(U.mesh)
    ctx.bind_bcs(U(), U.bcs, 0)
    if not carried:
        ctx.project_correct(U(), p()[0], dt / rho, U.bcs)
        return report
    rot = form == "rotational"
    ctx.project_update(U(), x()[0], dt / rho, p()[0], nrhs[0] if rot else None, float(nu) * dt if rot else 0.0, U.bcs)
    p.apply_bcs()
    return report


def _source_tensor(ctx: Any, U: Field, srcs: list | None) -> Tensor:
    """the per-component sources ``_momentum_args`` resolved, as the work tensor S (d, *n): zeros where there is none"""
    S = ctx.work("projection S", U.dim)
    S.zero_()
    for c, e in enumerate(srcs or ()):
        if isinstance(e, Tensor):
            S[c].copy_(e.reshape(S[c].shape))
        elif e is not None:
            S[c].fill_(float(e))
    return S


def ns_step(U: Field, p: Field, nu: float | Tensor | Field, dt: float, config: dict | None = None, order: int = 3, *,
            rho: float = 1.0, source: Tensor | Field | tuple | list | None = None, solver: dict | None = None,
            form: str = "chorin", phi: Field | None = None) -> dict:
    """One step of the incompressible Navier-Stokes equations.  ``form`` "chorin" (the default), Chorin's non-incremental
    form: ``momentum_step(U, nu, dt, config, order, source=source)``, then ``project(U, p, dt, rho, solver)``.  "incremental"
    and "rotational": the seven statements of the module docstring -- the predictor feels ``-grad(p) / rho``, the solve is
    for the increment ``phi`` (None: built once from ``p``'s BCs, kept on ``p``), ``p`` is updated -- which hold a balanced
    state (``source = grad(p) / rho`` on a fluid at rest) bit for bit.  ``U``'s time advances by ``dt``; returns the solver's
    report.  Every check of both halves is made before a device is touched."""
    _project_args(U, p, dt, rho, form, phi, nu, "ns_step")
    if form == "chorin":
        momentum_step(U, nu, dt, config, order, source=source)
    else:
        _, _, srcs = _momentum_args(U, config, order, None, source, "ns_step")
        _diffusivity_of(_Component(U), nu, config, "ns_step")
        require_gpu(U(), "ns_step")
        ctx = context_for(U.mesh)
        if not U().is_contiguous():
            U.set_var_tensor(U().contiguous())
        p.apply_bcs()
        S = _source_tensor(ctx, U, srcs)
        src = ctx.work("projection src", U.dim)
        ctx.bind_bcs(U(), U.bcs, 0)                          # the interior set is that of U's faces
        ctx.project_correct(S, p()[0], 1.0 / float(rho), None, out=src)
        momentum_step(U, nu, dt, config, order, source=src)
    report = _project(U, p, float(dt), float(rho), solver, form, phi, nu, "ns_step")
    if hasattr(U, "_t"):
        U.update_time(dt)
    return report


def flow_stats(U: Field, dt: float | None = None) -> dict:
    """The diagnostics of a time loop, of the vector Field ``U`` in ONE pass (``pa_flow_stats``; ``U.apply_bcs()`` runs
    first): ``rate`` = max over all nodes of sum_a |U_a| / dx_a, ``div_max`` = max |div(U)| and ``div_sq`` = sum div(U)^2 over
    the interior set (``divergence``'s values), ``ke_sq`` = sum over all nodes of |U|^2; a NaN in ``U`` makes the maximum it
    contributes to NaN.  With ``dt`` also ``cfl = dt * rate``, ``div_l2 = sqrt(div_sq * cell volume)`` and ``ke = 0.5 * ke_sq *
    cell volume``.  Synchronises."""
    _vector_args(U, "flow_stats")
    _number("dt", dt, "flow_stats", optional=True)
    require_gpu(U(), "flow_stats")
    if not U().is_contiguous():
        U.set_var_tensor(U().contiguous())
    U.apply_bcs()
    rate, div_max, div_sq, ke_sq = context_for(U.mesh).flow_stats(U())
    out = {"rate": rate, "div_max": div_max, "div_sq": div_sq, "ke_sq": ke_sq}
    if dt is not None:
        vol = math.prod(float(h) for h in U.mesh.dx_list)
        out.update(cfl=float(dt) * rate, div_l2=math.sqrt(div_sq * vol), ke=0.5 * ke_sq * vol)
    return out


def ns_march(U: Field, p: Field, nu: float | Tensor | Field, dt: float, nsteps: int, config: dict | None = None, order: int = 3,
             *, rho: float = 1.0, source: Tensor | Field | tuple | list | None = None, solver: dict | None = None,
             form: str = "incremental", phi: Field | None = None, cfl: float | None = None) -> dict:
    """``nsteps`` steps of ``ns_step`` (a Python loop: every step solves).  ``cfl`` a positive number: step k takes
    ``dt_k = min(dt, cfl / rate_k)`` with ``rate_k`` from ``flow_stats`` before the step, which fills ``U``'s faces (``dt``
    when the fluid is at rest); a
    rate that is not finite raises ``RuntimeError`` and names the step.  Returns ``{"steps", "t", "dt": [...], "itr": [...],
    "converge": [...]}``: the steps taken, the time covered, and per step its dt and the solver's report."""
    _project_args(U, p, dt, rho, form, phi, nu, "ns_march")
    if isinstance(nsteps, bool) or not isinstance(nsteps, int):
        raise TypeError(f"pyapes_amd: ns_march: nsteps is an int (got {type(nsteps).__name__})")
    if nsteps < 0:
        raise ValueError(f"pyapes_amd: ns_march: nsteps = {nsteps!r} (not negative)")
    _number("cfl", cfl, "ns_march", optional=True)
    if cfl is not None and not math.isfinite(cfl):
        raise ValueError(f"pyapes_amd: ns_march: cfl = {cfl!r} (a positive number)")
    _momentum_args(U, config, order, None, source, "ns_march")
    _diffusivity_of(_Component(U), nu, config, "ns_march")
    out: dict[str, Any] = {"steps": 0, "t": 0.0, "dt": [], "itr": [], "converge": []}
    for k in range(nsteps):
        dt_k = float(dt)
        if cfl is not None:
            rate = flow_stats(U)["rate"]
            if not math.isfinite(rate):
                raise RuntimeError(f"pyapes_amd: ns_march: step {k}: the CFL rate of U is {rate!r}")
            if rate > 0.0:
                dt_k = min(dt_k, float(cfl) / rate)
        rep = ns_step(U, p, nu, dt_k, config, order, rho=rho, source=source, solver=solver, form=form, phi=phi)
        out["steps"] += 1
        out["t"] += dt_k
        out["dt"].append(dt_k)
        out["itr"].append(rep["itr"])
        out["converge"].append(rep["converge"])
    return out
