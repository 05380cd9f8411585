"""Explicit time marching (new; the reference's ``Ddt`` is a stub).

``euler_step(phi, u, nu, dt, fdm_config)``:  phi <- B( phi + dt * ( nu * lap(phi) - div(u phi) ) )
on the interior set, lap / div being the explicit operators (edge=False) evaluated on the current,
BC-filled phi.  One fused kernel (``k_euler``) + the ordered BC fill.

``rk_step`` / ``rk_march``: strong-stability-preserving Runge-Kutta steps of order 1, 2, 3 in Shu-Osher form -- every
stage is the Euler step E followed by a convex combination with the state the step started from, ``c0 phi0 + c1 E(phi_s)``,
formed inside the step kernel (``Context.rk_stage``).  Order 3 marches central ``Div`` without diffusion up to CFL sqrt(3).

Self-advection, ``div(phi, phi)`` (Burgers' term): pass the field itself as ``u`` -- ``euler_march(phi, phi, ...)``,
``rk_march(phi, phi, ...)`` -- or a Tensor / Field on ``phi()``'s own storage (``advects_itself``).  Every step and every
stage is then advected by ITS OWN input, ``B(c0 phi0 + c1 E_self(phi_s))`` with the speed ``phi_s``, through
``Context.rk_march_self``.  A clone of ``phi`` is a speed frozen at the start of the call, as any other tensor.

Source term, ``source=S`` (keyword only) on all four entry points:  d(phi)/dt = nu lap(phi) - div(u phi) + S.  On the interior
set  a = nu*lap; a = a - adv; a = a + s; a = dt*a; v = phi + a,  every operation rounded in the mesh dtype, inside the step
kernel; a Runge-Kutta stage is ``B(c0 phi0 + c1 E_S(phi_s))`` with the source in every stage.  ``S`` is a float / int, a Tensor
shaped like ``phi()`` or like one component, or a scalar Field on the same mesh.  It is FROZEN for the whole call: a forcing
that depends on time is supplied anew per ``rk_step``.  ``None`` is the call without the argument, bit for bit.

Velocity: ``u`` with one advection speed per mesh axis, (u_0, .., u_{d-1}), on all four entry points -- uniform flow along one
axis, shear, rotation.  A float, a ``(1, *n)`` Tensor or a scalar Field stays ONE speed used on every axis (transport along the
diagonal); a velocity is
  * a tuple / list of ``mesh.dim`` entries, each a number or a Tensor of one component's shape (``phi()[0].shape``), of the
    mesh dtype and on the mesh device -- if any entry is a Tensor the numeric entries are materialised on the host side as
    tensors filled with the number (all-numeric velocities stay scalars down to the kernel),
  * a Tensor of shape ``(mesh.dim, *n)`` on a mesh with more than one axis, or
  * a vector Field with ``dim == mesh.dim > 1`` on the same mesh.
Per axis the scheme's own term is formed with that axis's component (DESIGN.md section 4 "Velocity"): upwind and QUICK in the
advective form u . grad(phi) with the speed at the node, central in the conservative form with u_a at the axis's two
neighbours.  The velocity is FROZEN for the whole call, like a speed tensor; ``source=`` composes with it.  Not with a velocity:
slab and axisymmetric meshes, ``compat: True``, a component on ``phi``'s own storage (no self-advection by component).

Momentum: ``momentum_step`` / ``momentum_march`` march a VECTOR field ``U`` with ``U.dim == mesh.dim >= 2`` that advects itself,
    dU_c/dt = nu lap(U_c) - (U . grad) U_c + S_c,
the momentum predictor of a projection step (DESIGN.md section 4 "Momentum").  Component c of a stage is the velocity step
above applied to the scalar V_c with the velocity (V_0, .., V_{d-1}), all components of the stage's INPUT V, then the BC fill
with component c's face values; every Runge-Kutta stage is advected by its own input and no component sees another
component's output of the same stage.  ``u=`` a velocity transports every component by that frozen velocity instead (the
linearised, Oseen form: ``mesh.dim`` scalar marches in one call); ``source=`` has one entry per component.  The four scalar
entry points keep refusing vector targets.

Diffusivity field: ``nu`` a Tensor shaped like ``phi()`` or like one component, or a scalar Field on the same mesh, on all six
entry points -- two materials, a conductivity that depends on position, an eddy viscosity under ``momentum_march`` (one field for
every component).  ``nu lap(phi)`` is then replaced by the conservative ``div(nu grad phi)`` with the diffusivity averaged onto
the faces (DESIGN.md section 4 "Diffusivity field"): per axis  t = ((nu[+1] + nu) (x[+1] - x) - (nu + nu[-1]) (x - x[-1])) * 0.5/dx^2,
every operation rounded on its own; the step reads the BC-filled face values of its input and ``nu`` at every node the stencil
touches (``nu`` has no BCs).  ``nu`` is FROZEN for the call, and it composes with ``source=``, a velocity, self-advection and every
limiter.  A number is the path it always was, bit for bit.  Not with a diffusivity field: slab and axisymmetric meshes,
``compat: True``, ``nu`` on ``phi``'s own storage.
"""
from __future__ import annotations

from typing import Any

import torch
from torch import Tensor

from ..backend import require_gpu
from ..hip.context import context_for
from ..variables import Field
from .fdc import _adv_of, div_kind, quick_mesh_check


# (c0, c1) of every FUSED stage of a step, in order; the plain Euler stage phi1 = E(phi0) in front of them is implied.
#   order 2:  phi' = 1/2 phi0 + 1/2 E(phi1)
#   order 3:  phi2 = 3/4 phi0 + 1/4 E(phi1);  phi' = 1/3 phi0 + 2/3 E(phi2)
SSP_STAGES: dict[int, list[tuple[float, float]]] = {
    1: [],
    2: [(0.5, 0.5)],
    3: [(3.0 / 4.0, 1.0 / 4.0), (1.0 / 3.0, 2.0 / 3.0)],
}


def advects_itself(phi: Field, u: Any) -> bool:
    """``u`` is ``phi`` -- the same Field object, or a Tensor / Field whose storage is ``phi()``'s own (same ``data_ptr``,
    same shape) -- so the march advects the field by itself.  A clone is not: it stays what it was."""
    if u is phi:
        return True
    t = u() if isinstance(u, Field) else u
    if not isinstance(t, Tensor):
        return False
    p = phi()
    return t.data_ptr() == p.data_ptr() and tuple(t.shape) == tuple(p.shape)


def _no_self_on_slabs(phi: Field, what: str) -> None:
    if getattr(phi.mesh, "slab", None) is not None:
        raise NotImplementedError(f"pyapes_amd: {what}: self-advection on a slab mesh (single GPU only)")


def _source_of(phi: Field, source: Any, what: str) -> float | Tensor | None:
    """the checks of ``source=`` -- made before a device is touched -- and what the Context methods take: None, a float or
    a contiguous tensor of one component's shape"""
    if source is None:
        return None
    mesh = phi.mesh
    if getattr(mesh, "slab", None) is not None:
        raise NotImplementedError(f"pyapes_amd: {what}: a source term on a slab mesh (single GPU only)")
    if mesh.coord_sys == "rz":
        raise NotImplementedError(f"pyapes_amd: {what}: a source term on an axisymmetric (rz) mesh")
    if isinstance(source, Field):
        if source.dim != 1:
            raise NotImplementedError(f"pyapes_amd: {what}: the source is a scalar field (got {source.dim} components)")
        if source.mesh is not mesh:
            raise ValueError(f"pyapes_amd: {what}: the source Field lives on another mesh")
        source = source()
    if isinstance(source, bool):
        raise TypeError(f"pyapes_amd: {what}: source is a float, a Tensor or a scalar Field")
    if isinstance(source, (float, int)):
        return float(source)
    if not isinstance(source, Tensor):
        raise TypeError(f"pyapes_amd: {what}: source is a float, a Tensor or a scalar Field (got {type(source).__name__})")
    p = phi()
    if tuple(source.shape) == tuple(p.shape):
        source = source[0]
    elif phi.dim != 1 or tuple(source.shape) != tuple(p.shape[1:]):
        raise ValueError(f"pyapes_amd: {what}: source shape {tuple(source.shape)}, expected {tuple(p.shape)} or {tuple(p.shape[1:])}")
    if source.dtype != p.dtype:
        raise ValueError(f"pyapes_amd: {what}: source dtype {source.dtype} != mesh dtype {p.dtype}")
    if source.device != p.device:
        raise ValueError(f"pyapes_amd: {what}: source on {source.device}, the field on {p.device}")
    if source.untyped_storage().data_ptr() == p.untyped_storage().data_ptr():
        raise ValueError(f"pyapes_amd: {what}: the source shares phi's storage (the step kernels read it while they write phi)")
    return source.contiguous()


def _diffusivity_of(phi: Any, nu: Any, config: dict | None, what: str) -> Any:
    """the checks of a diffusivity FIELD -- made before a device is touched -- and what the Context methods take: a contiguous
    tensor of one component's shape.  A number is handed back as it came: today's path, untouched."""
    if not isinstance(nu, (Tensor, Field)):
        return nu
    mesh = phi.mesh
    if getattr(mesh, "slab", None) is not None:
        raise NotImplementedError(f"pyapes_amd: {what}: a diffusivity field on a slab mesh (single GPU only)")
    if mesh.coord_sys == "rz":
        raise NotImplementedError(f"pyapes_amd: {what}: a diffusivity field on an axisymmetric (rz) mesh")
    if bool(((config or {}).get("div") or {}).get("compat", False)):
        raise NotImplementedError(f"pyapes_amd: {what}: a diffusivity field with compat: True (the reference's literal upwind form)")
    if isinstance(nu, Field):
        if nu.dim != 1:
            raise NotImplementedError(f"pyapes_amd: {what}: the diffusivity is a scalar field (got {nu.dim} components)")
        if nu.mesh is not mesh:
            raise ValueError(f"pyapes_amd: {what}: the diffusivity Field lives on another mesh")
        nu = nu()
    p = phi()
    comp = tuple(p.shape[1:])
    if tuple(nu.shape) == (1, *comp):
        nu = nu[0]
    elif tuple(nu.shape) != comp:
        raise ValueError(f"pyapes_amd: {what}: nu shape {tuple(nu.shape)}, expected {(1, *comp)} or {comp}")
    if nu.dtype != p.dtype:
        raise ValueError(f"pyapes_amd: {what}: nu dtype {nu.dtype} != mesh dtype {p.dtype}")
    if nu.device != p.device:
        raise ValueError(f"pyapes_amd: {what}: nu on {nu.device}, the field on {p.device}")
    if nu.untyped_storage().data_ptr() == p.untyped_storage().data_ptr():
        raise ValueError(f"pyapes_amd: {what}: nu shares phi's storage (the step kernels read it while they write phi; "
                         "nu does not depend on phi within a call)")
    return nu.contiguous()


def _velocity_of(phi: Field, u: Any, config: dict | None, what: str) -> list[float | Tensor] | None:
    """``u`` as a velocity -- one entry per mesh axis, all numbers or all contiguous tensors of one component's shape -- or None
    when ``u`` is one speed for every axis (a float, a ``(1, *n)`` Tensor, a scalar Field: the existing path, untouched).  All
    checks of a velocity are made here, before a device is touched."""
    mesh = phi.mesh
    nd = mesh.dim
    if phi.dim != 1 and not isinstance(u, (tuple, list)):
        return None   # a vector target with a Tensor / Field: refused where it is today ("... is for scalar fields")
    if isinstance(u, Field):
        if not (u.dim == nd and nd > 1):
            return None
        if u.mesh is not mesh:
            raise ValueError(f"pyapes_amd: {what}: the velocity Field lives on another mesh")
        t = u()
        entries: list[Any] = [t[a] for a in range(nd)]
    elif isinstance(u, Tensor):
        if not (nd > 1 and u.dim() == nd + 1 and u.shape[0] == nd):
            return None
        entries = [u[a] for a in range(nd)]
    elif isinstance(u, (tuple, list)):
        entries = list(u)
        if len(entries) != nd:
            raise ValueError(f"pyapes_amd: {what}: a velocity has one entry per mesh axis ({len(entries)} given, the mesh has {nd})")
    else:
        return None
    if phi.dim != 1:
        raise NotImplementedError(f"pyapes_amd: {what}: a velocity advects a scalar field (got {phi.dim} components)")
    if getattr(mesh, "slab", None) is not None:
        raise NotImplementedError(f"pyapes_amd: {what}: a velocity on a slab mesh (single GPU only)")
    if mesh.coord_sys == "rz":
        raise NotImplementedError(f"pyapes_amd: {what}: a velocity on an axisymmetric (rz) mesh")
    if bool(((config or {}).get("div") or {}).get("compat", False)):
        raise NotImplementedError(f"pyapes_amd: {what}: a velocity with compat: True (the reference's literal upwind form takes one speed)")
    p = phi()
    comp_shape = tuple(p.shape[1:])
    out: list[float | Tensor] = []
    for a, e in enumerate(entries):
        if isinstance(e, bool) or not isinstance(e, (float, int, Tensor)):
            raise TypeError(f"pyapes_amd: {what}: velocity entry {a} is a number or a Tensor (got {type(e).__name__})")
        if isinstance(e, Tensor):
            if tuple(e.shape) != comp_shape:
                raise ValueError(f"pyapes_amd: {what}: velocity entry {a} has shape {tuple(e.shape)}, expected {comp_shape}")
            if e.dtype != p.dtype:
                raise ValueError(f"pyapes_amd: {what}: velocity entry {a} has dtype {e.dtype}, the mesh {p.dtype}")
            if e.device != p.device:
                raise ValueError(f"pyapes_amd: {what}: velocity entry {a} on {e.device}, the field on {p.device}")
            if e.untyped_storage().data_ptr() == p.untyped_storage().data_ptr():
                raise ValueError(f"pyapes_amd: {what}: velocity entry {a} shares phi's storage (no self-advection by component)")
            out.append(e)
        else:
            out.append(float(e))
    if any(isinstance(e, Tensor) for e in out):   # mixed: the numbers become filled tensors
        out = [e.contiguous() if isinstance(e, Tensor) else torch.full(comp_shape, e, dtype=p.dtype, device=p.device) for e in out]
    return out


def _kind_of(config: dict | None, mesh: Any, what: str) -> int:
    """the Div kind ``config`` asks for (default: upwind), checked against the mesh where the scheme needs it (QUICK)"""
    cfg = (config or {}).get("div", {"limiter": "upwind"})
    kind = div_kind(cfg.get("limiter", "upwind").lower(), bool(cfg.get("compat", False)))
    quick_mesh_check(kind, mesh, what)
    return kind


def _run(ctx: Any, phi: Field, bufs: list[Tensor], order: int, kind: int, u: Any, vel: list[float | Tensor] | None,
         self_adv: bool, nu: float, dt: float, nsteps: int, src: float | Tensor | None) -> None:
    """``nsteps`` steps of ``order`` of ``phi`` over the work buffers ``bufs`` (``(1, *n)`` each; one: the Euler march), through
    the Context method that takes ``u`` -- a velocity, the field itself, else one speed.  ``phi`` adopts the buffer that holds
    the result."""
    w1 = bufs[0][0]
    w2 = None if len(bufs) == 1 or order == 1 else bufs[1][0]   # order 1: the ping-pong of two buffers
    if isinstance(nu, Tensor):   # a diffusivity field: one entry for every kind of speed (None: the field itself)
        speed = vel if vel is not None else (None if self_adv else _adv_of(u, phi))
        final = ctx.march_nu(phi()[0], w1, w2, order, kind, speed, nu, dt, nsteps, source=src)
    elif vel is not None:
        final = ctx.rk_march_vel(phi()[0], w1, w2, order, kind, vel, nu, dt, nsteps, source=src)
    elif self_adv:   # the speed moves with the field: no single pointer names it
        final = ctx.rk_march_self(phi()[0], w1, w2, order, kind, nu, dt, nsteps, source=src)
    elif len(bufs) == 1:
        final = ctx.euler_march(phi()[0], w1, kind, _adv_of(u, phi), nu, dt, nsteps, source=src)
    else:
        final = ctx.rk_march(phi()[0], w1, bufs[1][0], order, kind, _adv_of(u, phi), nu, dt, nsteps, source=src)
    for w in bufs:
        if final.data_ptr() == w[0].data_ptr():
            phi.set_var_tensor(w)


def _march_on_slabs(phi: Field, u: Any, nu: float, dt: float, nsteps: int, kind: int) -> Field:
    """``Mesh(..., slab=(rank, world))``: the same call on every rank of the process group (pyapes_amd/slab.py SlabEuler)."""
    import torch.distributed as dist

    from ..slab import SlabEuler
    if not dist.is_initialized():
        raise RuntimeError("pyapes_amd: a march on a slab mesh needs torch.distributed to be initialised "
                           "(one process per GPU, backend 'nccl' = RCCL)")
    backend = context_for(phi.mesh)
    if not getattr(backend, "is_standin", False):
        require_gpu(phi(), "euler_march")
    if not phi().is_contiguous():
        phi.set_var_tensor(phi().contiguous())
    adv = _adv_of(u, phi)
    final = SlabEuler(phi.mesh, phi, dist, backend=backend).march(kind, adv, nu, dt, nsteps)
    if final.data_ptr() != phi()[0].data_ptr():
        phi.set_var_tensor(final.unsqueeze(0))
    return phi


def euler_step(phi: Field, u: float | Tensor | Field | tuple | list, nu: float | Tensor | Field, dt: float,
               config: dict | None = None, *, source: float | Tensor | Field | None = None) -> Field:
    """Advance ``phi`` in place by one explicit Euler step; returns ``phi``.  ``source``: the term S of ``+ S`` (module
    docstring), frozen for the call.  ``u``: one speed for every axis, or a velocity -- one speed per mesh axis (module
    docstring "Velocity"), frozen for the call."""
    vel = _velocity_of(phi, u, config, "euler_step")
    src = _source_of(phi, source, "euler_step")
    nu = _diffusivity_of(phi, nu, config, "euler_step")
    kind = _kind_of(config, phi.mesh, "euler_step")
    if getattr(phi.mesh, "slab", None) is not None:
        return _march_on_slabs(phi, u, nu, dt, 1, kind)
    require_gpu(phi(), "euler_step")
    if phi.dim != 1:
        raise NotImplementedError("pyapes_amd: euler_step is for scalar fields")
    ctx = context_for(phi.mesh)
    ctx.bind_bcs(phi(), phi.bcs, 0)
    out = torch.empty_like(phi())
    if isinstance(nu, Tensor):
        ctx.step_nu(phi()[0], None, out[0], 0.0, 0.0, kind, vel if vel is not None else _adv_of(u, phi), nu, dt, source=src)
    elif vel is not None:
        ctx.euler_step_vel(phi()[0], out[0], kind, vel, nu, dt, source=src)
    else:
        ctx.euler_step(phi()[0], out[0], kind, _adv_of(u, phi), nu, dt, source=src)
    phi.set_var_tensor(out)
    return phi


def euler_march(phi: Field, u: float | Tensor | Field | tuple | list, nu: float | Tensor | Field, dt: float, nsteps: int,
                config: dict | None = None, *, source: float | Tensor | Field | None = None) -> Field:
    """``nsteps`` explicit Euler steps with no host work in between (the whole march is enqueued by one
    C-ABI call: fused step kernel + ordered BC fill per step, ping-pong buffers).  ``source``: the term S of ``+ S``
    (module docstring), frozen for the whole call -- the same S in every step.  ``u`` may be a velocity, one speed per mesh
    axis (module docstring "Velocity"): it is FROZEN for the whole call, like a speed tensor."""
    if phi.dim != 1:
        raise NotImplementedError("pyapes_amd: euler_march is for scalar fields")
    vel = _velocity_of(phi, u, config, "euler_march")
    src = _source_of(phi, source, "euler_march")
    nu = _diffusivity_of(phi, nu, config, "euler_march")
    kind = _kind_of(config, phi.mesh, "euler_march")
    self_adv = advects_itself(phi, u)
    if self_adv:
        _no_self_on_slabs(phi, "euler_march")
    if getattr(phi.mesh, "slab", None) is not None:
        phi = _march_on_slabs(phi, u, nu, dt, nsteps, kind)
        if hasattr(phi, "_t"):
            phi.update_time(dt * nsteps)
        return phi
    require_gpu(phi(), "euler_march")
    ctx = context_for(phi.mesh)
    ctx.bind_bcs(phi(), phi.bcs, 0)
    if not phi().is_contiguous():
        phi.set_var_tensor(phi().contiguous())
    _run(ctx, phi, [torch.empty_like(phi())], 1, kind, u, vel, self_adv, nu, dt, nsteps, src)
    if hasattr(phi, "_t"):
        phi.update_time(dt * nsteps)
    return phi


def _rk_args(phi: Field, config: dict | None, order: int, what: str) -> int:
    """the checks every Runge-Kutta entry makes before it touches a device; returns the Div kind"""
    if order not in SSP_STAGES:
        raise ValueError(f"pyapes_amd: {what}: order {order!r} (1, 2 or 3)")
    if phi.dim != 1:
        raise NotImplementedError(f"pyapes_amd: {what} is for scalar fields")
    if getattr(phi.mesh, "slab", None) is not None:
        raise NotImplementedError(f"pyapes_amd: {what} on a slab mesh (the stages march on one GPU; euler_march does slabs)")
    return _kind_of(config, phi.mesh, what)


def rk_step(phi: Field, u: float | Tensor | Field | tuple | list, nu: float | Tensor | Field, dt: float, config: dict | None = None,
            order: int = 3, *, source: float | Tensor | Field | None = None) -> Field:
    """Advance ``phi`` by one SSP Runge-Kutta step of ``order`` (1: the Euler step); returns ``phi``.  ``source``: the term S
    of ``+ S`` (module docstring), the same in every stage of the step; a forcing that depends on time is handed in anew
    with each call.  ``u`` may be a velocity (module docstring "Velocity"), frozen for the step."""
    vel = _velocity_of(phi, u, config, "rk_step")
    kind = _rk_args(phi, config, order, "rk_step")
    src = _source_of(phi, source, "rk_step")
    nu = _diffusivity_of(phi, nu, config, "rk_step")
    if order == 1:
        return euler_step(phi, u, nu, dt, config, source=src)   # (a speed on phi's own storage is self-advection at the C ABI)
    self_adv = advects_itself(phi, u)
    require_gpu(phi(), "rk_step")
    ctx = context_for(phi.mesh)
    ctx.bind_bcs(phi(), phi.bcs, 0)
    if not phi().is_contiguous():
        phi.set_var_tensor(phi().contiguous())
    _run(ctx, phi, [torch.empty_like(phi()), torch.empty_like(phi())], order, kind, u, vel, self_adv, nu, dt, 1, src)
    return phi


def rk_march(phi: Field, u: float | Tensor | Field | tuple | list, nu: float | Tensor | Field, dt: float, nsteps: int,
             config: dict | None = None, order: int = 3, *, source: float | Tensor | Field | None = None) -> Field:
    """``nsteps`` SSP Runge-Kutta steps of ``order`` with no host work in between (one C-ABI call enqueues the whole
    march: the Euler kernel, then one fused stage kernel per further stage, over three buffers).  Arguments as
    ``euler_march``; ``phi`` holds the final state on return and its time advances by ``nsteps * dt``.  ``u`` being
    ``phi`` itself (``advects_itself``) marches ``div(phi, phi)``: every stage is advected by its own input.  ``source``:
    the term S of ``+ S`` (module docstring), in every stage of every step and FROZEN for the whole call -- a forcing that
    depends on time is re-supplied per ``rk_step``.  ``u`` may be a velocity, one speed per mesh axis (module docstring
    "Velocity"): FROZEN for the whole call, the same in every stage of every step."""
    vel = _velocity_of(phi, u, config, "rk_march")
    kind = _rk_args(phi, config, order, "rk_march")
    src = _source_of(phi, source, "rk_march")
    nu = _diffusivity_of(phi, nu, config, "rk_march")
    self_adv = advects_itself(phi, u)
    require_gpu(phi(), "rk_march")
    ctx = context_for(phi.mesh)
    ctx.bind_bcs(phi(), phi.bcs, 0)
    if not phi().is_contiguous():
        phi.set_var_tensor(phi().contiguous())
    _run(ctx, phi, [torch.empty_like(phi()), torch.empty_like(phi())], order, kind, u, vel, self_adv, nu, dt, nsteps, src)
    if hasattr(phi, "_t"):
        phi.update_time(dt * nsteps)
    return phi


class _Component:
    """one component of a vector Field, as the scalar target ``_velocity_of`` / ``_source_of`` check against (a view of the
    vector's storage: an entry that shares it is caught)"""

    def __init__(self, U: Field):
        self.mesh, self.dim, self._t = U.mesh, 1, U()[0:1]

    def __call__(self) -> Tensor:
        return self._t


def _shares_storage(t: Any, p: Tensor) -> bool:
    t = t() if isinstance(t, Field) else t
    return isinstance(t, Tensor) and t.device == p.device and t.untyped_storage().data_ptr() == p.untyped_storage().data_ptr()


def _momentum_args(U: Field, config: dict | None, order: int, u: Any, source: Any,
                   what: str) -> tuple[int, list[float | Tensor] | None, list[float | Tensor | None] | None]:
    """every check of ``momentum_step`` / ``momentum_march``, made before a device is touched; returns the Div kind, the frozen
    velocity (None: ``U`` transports itself) and the per-component sources (None: no source)"""
    if order not in SSP_STAGES:
        raise ValueError(f"pyapes_amd: {what}: order {order!r} (1, 2 or 3)")
    mesh = U.mesh
    nd = mesh.dim
    if nd < 2:
        raise NotImplementedError(f"pyapes_amd: {what}: a 1-D mesh (a scalar that advects itself: rk_march(phi, phi, ...))")
    if U.dim != nd:
        raise NotImplementedError(f"pyapes_amd: {what}: a vector field with one component per mesh axis ({U.dim} for {nd})")
    if getattr(mesh, "slab", None) is not None:
        raise NotImplementedError(f"pyapes_amd: {what} on a slab mesh (single GPU only)")
    if mesh.coord_sys == "rz":
        raise NotImplementedError(f"pyapes_amd: {what} on an axisymmetric (rz) mesh")
    cfg = (config or {}).get("div", {"limiter": "upwind"})
    if bool(cfg.get("compat", False)):
        raise NotImplementedError(f"pyapes_amd: {what} with compat: True (the reference's literal upwind form takes one speed)")
    kind = _kind_of(config, mesh, what)
    comp = _Component(U)
    vel = None
    if u is not None:
        entries = list(u) if isinstance(u, (tuple, list)) else [u]
        if u is U or any(_shares_storage(e, U()) for e in entries):
            raise NotImplementedError(f"pyapes_amd: {what}: u= on U's own storage (u=None is the field that transports itself; "
                                      "a frozen velocity is a clone)")
        vel = _velocity_of(comp, u, config, what)
        if vel is None:
            raise TypeError(f"pyapes_amd: {what}: u= is a velocity, one entry per mesh axis (a tuple / list, a "
                            f"({nd}, *n) Tensor or a vector Field), or None")
    srcs = None
    if source is not None:
        p = U()
        if isinstance(source, Field):
            if source.mesh is not mesh:
                raise ValueError(f"pyapes_amd: {what}: the source Field lives on another mesh")
            if source.dim != nd:
                raise ValueError(f"pyapes_amd: {what}: the source Field has {source.dim} components, U {nd}")
            source = source()
        if isinstance(source, Tensor):
            if tuple(source.shape) != tuple(p.shape):
                raise ValueError(f"pyapes_amd: {what}: source shape {tuple(source.shape)}, expected {tuple(p.shape)}")
            source = [source[c] for c in range(nd)]
        if not isinstance(source, (tuple, list)):
            raise TypeError(f"pyapes_amd: {what}: source is None, a list / tuple of {nd} entries, a ({nd}, *n) Tensor or a "
                            f"vector Field (got {type(source).__name__})")
        if len(source) != nd:
            raise ValueError(f"pyapes_amd: {what}: the source has one entry per component ({len(source)} given, U has {nd})")
        srcs = [_source_of(comp, e, what) for e in source]
    return kind, vel, srcs


def _momentum(U: Field, nu: float | Tensor | Field, dt: float, nsteps: int, config: dict | None, order: int, u: Any, source: Any,
              what: str) -> Field:
    kind, vel, srcs = _momentum_args(U, config, order, u, source, what)
    nu = _diffusivity_of(_Component(U), nu, config, what)
    require_gpu(U(), what)
    ctx = context_for(U.mesh)
    if not U().is_contiguous():
        U.set_var_tensor(U().contiguous())
    ctx.bind_bcs(U(), U.bcs, 0)
    w1 = torch.empty_like(U())
    w2 = None if order == 1 else torch.empty_like(U())
    final = ctx.momentum_march(U(), w1, w2, order, kind, vel, nu, dt, nsteps, srcs, U.bcs)
    if final.data_ptr() != U().data_ptr():
        U.set_var_tensor(final)
    return U


def momentum_step(U: Field, nu: float | Tensor | Field, dt: float, config: dict | None = None, order: int = 3, *,
                  u: Tensor | Field | tuple | list | None = None, source: Tensor | Field | tuple | list | None = None) -> Field:
    """Advance the vector field ``U`` by one SSP Runge-Kutta step of ``order`` of the momentum equation (module docstring
    "Momentum"); returns ``U``, whose time is not advanced (as ``rk_step``).  ``u`` None: ``U`` transports itself, every stage by
    its own input; a velocity: every component is transported by it, frozen.  ``source``: None, one entry per component (each
    what a scalar march takes), a ``(dim, *n)`` Tensor or a vector Field on the same mesh -- frozen, in every stage.  BC values
    (callables included) are resolved once per call."""
    return _momentum(U, nu, dt, 1, config, order, u, source, "momentum_step")


def momentum_march(U: Field, nu: float | Tensor | Field, dt: float, nsteps: int, config: dict | None = None, order: int = 3, *,
                   u: Tensor | Field | tuple | list | None = None, source: Tensor | Field | tuple | list | None = None) -> Field:
    """``nsteps`` steps of ``momentum_step`` with no host work in between (one C-ABI call, ``pa_momentum_march``: per stage
    and component one step kernel and its BC fill, over three vector buffers); ``U`` holds the final state and its time
    advances by ``nsteps * dt``.  ``u``, ``source`` and the BC values are FROZEN for the whole call."""
    U = _momentum(U, nu, dt, nsteps, config, order, u, source, "momentum_march")
    if hasattr(U, "_t"):
        U.update_time(dt * nsteps)
    return U
