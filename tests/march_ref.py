"""The explicit marches restated on the CPU in torch, operation for operation what the device kernels compute (DESIGN.md
section 4), built on the oracle's Laplacian, Div tables, interior set and BC fill.  The one yardstick of the march tests, host
and GPU: the Euler step E, the Runge-Kutta stage and the march, with one advection speed or with a velocity, with every Div
limiter, with a diffusivity number or field, with and without a source, and the momentum march on top.

E on the interior set, every operation rounded on its own in the field's dtype:
    a = nu * lap;  a = a - adv;  [a = a + s;]  a = dt * a;  v = phi + a            (nu a number)
    a = d - adv;                 [a = a + s;]  a = dt * a;  v = phi + a            (nu a tensor: a DIFFUSIVITY FIELD)
s the source at the cell, or the scalar source rounded to the dtype; the ordered BC fill B follows.  Without a source the
``a + s`` operation does not exist, and with a number nu the result is bit-identical to ``oracle.euler_step``
(tests/test_source_host.py).  A stage is  B(c0 * phi0 + c1 * E(phi_s));  the speed (unless the field advects itself), nu and S
are frozen over a march.

``u`` decides the advection term.  A number or a field-shaped tensor is ONE speed for every axis, and adv is the oracle's own:
    "upwind"  div_upwind_intended;   "none" (central) and "compat" (the literal upwind form)  div_tables / apply_div.
A list / tuple of ``mesh.dim`` entries, each a number (rounded to the field's dtype) or a tensor of one component's shape, is a
VELOCITY, one speed u_a per mesh axis a, and adv = (+0) + t_0 + t_1 + ... of the per-axis terms
    upwind   t_a = (max(u_a,0) (x - x[-1]_a) + min(u_a,0) (x[+1]_a - x)) * fl(1/dx_a)                (upwind_term)
    central  the oracle's div_tables / apply_div on the field stacked mesh.dim times with the velocity as its advection
             tensor: cP = u_a[+1]_a, cC = 0 u_a, cM = -u_a[-1]_a, the periodic-face zeroing, / (2 dx_a)
The two forms are derived separately on purpose: that they agree for equal components is what tests/test_velocity_host.py
asserts.  "quick", "minmod" and "mc" are this file's per-axis terms for both forms (one speed: the same u_a on every axis).

QUICK, advective form, the speed taken at the node, u+ = max(u, 0), u- = min(u, 0); per mesh axis a:
    bq = 3/8 (x[+1] + x) - 7/8 x[-1] + 1/8 x[-2]        (with u+)
    fq = 7/8 x[+1] - 3/8 (x[-1] + x) - 1/8 x[+2]        (with u-)
    term_a = (u+ bq + u- fq) * fl(1 / dx_a);   adv = (+0) + term_0 + term_1 + term_2
every operation rounded on its own, in the order of the statements of quick_term.  Neighbours wrap around on every axis; on an
axis without a periodic face the half whose far-upwind node would wrap (bq at index <= 1, fq at index >= N - 2) is the central
difference 0.5 (x[+1] - x[-1]) instead.

The slope-limited (TVD) schemes, Div limiters "minmod" and "mc" (PA_OP_DIV_MINMOD = 6, PA_OP_DIV_MC = 7; include/pyapes_hip.h,
DESIGN.md section 4 "Bounded advection"), same form and speed halves; per mesh axis a, neighbours wrapping around:
    dm = x - x[-1];  dp = x[+1] - x;  dmm = x[-1] - x[-2];  dpp = x[+2] - x[+1]
    s0 = L(dm, dp);  sm = L(dmm, dm);  sp = L(dp, dpp)
    t = s0 - sm;  t = 0.5 t;  bq = dm + t            (with u+)
    t = sp - s0;  t = 0.5 t;  fq = dp - t            (with u-)
    p = u+ bq;  m = u- fq;  p = p + m;  term_a = p * fl(1 / dx_a);      adv = (+0) + term_0 + term_1 + term_2
L = minmod:  v = 0;  a, b >= 0: the smaller;  a, b < 0: the larger;  a * b <= 0: 0.     L = mc:  v = minmod(a, b); s = a + b;
minmod(2 v, s / 2).  On an axis without a periodic face the half whose far-upwind node would wrap is first-order upwind:
bq = dm at index <= 1, fq = dp at index >= N - 2.

The diffusivity field, the term d = div(nu grad phi) with nu per node (new, defined by this project, no reference counterpart;
DESIGN.md section 4 "Diffusivity field"); per mesh axis a:
    ih = fl(1 / dx_a);  w = ih * ih;  w = 0.5 * w
    nup = nu[+1]_a + nu;  num = nu + nu[-1]_a;  fp = x[+1]_a - x;  fm = x - x[-1]_a
    t = nup * fp;  s = num * fm;  t = t - s;  t = t * w;  d = d + t                  (d starts at +0, axes ascending)
Neighbours wrap around on every axis.  The step reads the BC-filled face values of its input, never the Neumann 2/3 rows of the
Laplacian tables, and nu at every node the stencil touches: nu has no BCs.

The momentum march -- a vector field U with one component per mesh axis that advects itself,
    dU_c/dt = nu lap(U_c) - (U . grad) U_c + S_c                  (div(nu grad U_c) with a diffusivity field)
-- is the namespace ``momentum``: per stage and component c the step / stage of the scalar V_c with the velocity
u = [V_0, .., V_{d-1}], ALL components of the stage's input V, so no component sees another component's output of the same
stage, and component c's oracle BCs.
"""
from __future__ import annotations

from typing import Callable, Sequence

import torch
from torch import Tensor

from pyapes_oracle import (apply_div, apply_laplacian, bc_fill, div_tables, div_upwind_intended, interior_slicer,
                           laplacian_tables)

SSP_STAGES = {1: [], 2: [(0.5, 0.5)], 3: [(3.0 / 4.0, 1.0 / 4.0), (1.0 / 3.0, 2.0 / 3.0)]}


# ---- the per-axis advection terms: (x, up, um, a, periodic, mesh[, limiter]) -> term_a --------------------------------
def upwind_term(x: Tensor, up: Tensor, um: Tensor, a: int, periodic: bool, mesh) -> Tensor:
    """term_a of the component ``x`` (*n) along mesh axis ``a`` with the speed halves ``up`` / ``um``"""
    inv = torch.ones((), dtype=x.dtype) / mesh.dx[a]
    bwd = x - torch.roll(x, 1, a)
    fwd = torch.roll(x, -1, a) - x
    t = up * bwd
    m = um * fwd
    t = t + m
    t = t * inv
    return t


def quick_halves(x: Tensor, a: int, periodic: bool) -> tuple[Tensor, Tensor]:
    """(bq, fq) of the component ``x`` (*n) along mesh axis ``a``"""
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
    if not periodic:
        cen = xp - xm
        cen = 0.5 * cen
        idx = torch.arange(n).reshape([n if q == a else 1 for q in range(x.dim())])
        bq = torch.where(idx <= 1, cen, bq)
        fq = torch.where(idx >= n - 2, cen, fq)
    return bq, fq


def quick_term(x: Tensor, up: Tensor, um: Tensor, a: int, periodic: bool, mesh) -> Tensor:
    bq, fq = quick_halves(x, a, periodic)
    inv = torch.ones((), dtype=x.dtype) / mesh.dx[a]
    p = up * bq
    m = um * fq
    p = p + m
    p = p * inv
    return p


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


def tvd_halves(x: Tensor, a: int, periodic: bool, limiter) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """(bq, fq, dm, dp) of the component ``x`` (*n) along mesh axis ``a``; ``limiter`` a name of LIMITERS or a slope L(a, b)"""
    L = limiter if callable(limiter) else LIMITERS[limiter]
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
    bq, fq, _, _ = tvd_halves(x, a, periodic, limiter)
    inv = torch.ones((), dtype=x.dtype) / mesh.dx[a]
    p = up * bq
    m = um * fq
    p = p + m
    p = p * inv
    return p


# ---- the advection term ---------------------------------------------------------------------------------------------
def components(u: Sequence, phi: Tensor) -> list[Tensor]:
    """the velocity as one tensor of a component's shape per mesh axis (a number: filled, i.e. rounded to the dtype)"""
    nd = phi.dim() - 1
    assert len(u) == nd, "a velocity has one entry per mesh axis"
    out = []
    for e in u:
        if isinstance(e, Tensor):
            assert e.shape == phi[0].shape and e.dtype == phi.dtype
            out.append(e)
        else:
            out.append(torch.full_like(phi[0], float(e)))
    return out


def sum_axes(term, u, phi: Tensor, mesh, bcs: Sequence, *args) -> Tensor:
    """(1, *n): (+0) + term_0 + term_1 + ... at EVERY node of the scalar field ``phi`` (1, *n); ``u`` a velocity, or one
    speed (a float or a field-shaped tensor) for every axis"""
    assert phi.shape[0] == 1
    x = phi[0]
    if isinstance(u, (list, tuple)):
        speeds = components(u, phi)
    elif isinstance(u, Tensor):
        assert u.shape == phi.shape, "a speed tensor is field-shaped"
        speeds = [u[0]] * mesh.dim
    else:
        speeds = [torch.full_like(x, float(u))] * mesh.dim
    periodic = [False] * mesh.dim
    for bc in bcs or []:
        if bc.type == "periodic":
            periodic[mesh.axis_of(bc.face)] = True
    zeros = torch.zeros_like(x)
    out = torch.zeros_like(x)
    for a, ua in enumerate(speeds):
        up, um = torch.max(ua, zeros), torch.min(ua, zeros)
        out = out + term(x, up, um, a, periodic[a], mesh, *args)
    return out.unsqueeze(0)


def div_quick(u, var: Tensor, mesh, bcs: Sequence) -> Tensor:
    return sum_axes(quick_term, u, var, mesh, bcs)


def div_tvd(u, var: Tensor, mesh, bcs: Sequence, limiter) -> Tensor:
    return sum_axes(tvd_term, u, var, mesh, bcs, limiter)


def adv_tvd(u: Sequence, phi: Tensor, mesh, bcs: Sequence, limiter) -> Tensor:
    return sum_axes(tvd_term, list(u), phi, mesh, bcs, limiter)


def adv_upwind(u: Sequence, phi: Tensor, mesh) -> Tensor:
    return sum_axes(upwind_term, list(u), phi, mesh, None)


def adv_central(u: Sequence, phi: Tensor, mesh, bcs: Sequence) -> Tensor:
    nd = mesh.dim
    stacked = phi[0].unsqueeze(0).repeat(nd, *([1] * nd))
    vel = torch.stack(components(u, phi))
    return apply_div(div_tables(vel, stacked, mesh, bcs, "none"), stacked, nd)


def advection(phi: Tensor, u, mesh, bcs: Sequence, limiter) -> Tensor:
    """(1, *n): adv of the scalar field ``phi`` (1, *n) at every node, as the Euler step reads it"""
    velocity = isinstance(u, (list, tuple))
    if limiter == "quick":
        return sum_axes(quick_term, u, phi, mesh, bcs)
    if callable(limiter) or limiter in LIMITERS:
        return sum_axes(tvd_term, u, phi, mesh, bcs, limiter)
    if limiter == "upwind":
        return adv_upwind(u, phi, mesh) if velocity else div_upwind_intended(u, phi, mesh)
    if limiter == "none":
        return adv_central(u, phi, mesh, bcs) if velocity else apply_div(div_tables(u, phi, mesh, bcs, "none"), phi, mesh.dim)
    if limiter == "compat" and not velocity:   # the reference's literal upwind form (Div limiter "upwind" with compat=True)
        return apply_div(div_tables(u, phi, mesh, bcs, "upwind"), phi, mesh.dim)
    raise ValueError(limiter)


# ---- the diffusion term ---------------------------------------------------------------------------------------------
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


def diffusion(phi: Tensor, nu, mesh, bcs: Sequence) -> Tensor:
    """(1, *n): d for a diffusivity field, nu * lap on the oracle's Laplacian tables for a number"""
    if isinstance(nu, Tensor):
        return nu_term(phi, nu, mesh)
    return nu * apply_laplacian(laplacian_tables(phi, mesh, bcs), phi, mesh.dim)


# ---- the step, the stage and the march ------------------------------------------------------------------------------
def operator_parts(phi: Tensor, u, nu: float, mesh, bcs: Sequence, limiter) -> tuple[Tensor, Tensor]:
    """(lap, adv) of the scalar field ``phi`` (1, *n) at every node, as the Euler step with a number nu reads them"""
    return apply_laplacian(laplacian_tables(phi, mesh, bcs), phi, mesh.dim), advection(phi, u, mesh, bcs, limiter)


def _source_at(S, phi: Tensor, sl):
    """the operand of ``a + s`` on the interior set: a tensor shaped like ``phi`` or like one component, or a scalar"""
    if isinstance(S, Tensor):
        s = S[0] if S.dim() == phi.dim() else S
        assert s.shape == phi[0].shape and s.dtype == phi.dtype
        return s[sl]
    return float(S)


def euler_step(phi: Tensor, u, nu, dt: float, mesh, bcs: Sequence, limiter="upwind", S=None) -> Tensor:
    """E: B( phi + dt * ((nu * lap - adv) [+ s]) ) on the interior set; ``nu`` a number, or a tensor: d in place of nu * lap"""
    assert phi.shape[0] == 1
    sl = interior_slicer(mesh.dim, bcs)
    a = diffusion(phi, nu, mesh, bcs)[0][sl]
    a = a - advection(phi, u, mesh, bcs, limiter)[0][sl]
    if S is not None:
        a = a + _source_at(S, phi, sl)
    a = dt * a
    new = phi.clone()
    new[0][sl] = phi[0][sl] + a
    bc_fill(new, bcs)
    return new


def rk_stage(phi: Tensor, phi0: Tensor, c0: float, c1: float, u, nu, dt: float, mesh, bcs: Sequence, limiter="upwind",
             S=None, step=euler_step) -> Tensor:
    """``step``: the Euler step E, called as euler_step is (``oracle.euler_step``, which knows no source, is one)"""
    e = step(phi, u, nu, dt, mesh, bcs, limiter, *(() if S is None else (S,)))
    out = (c0 * phi0) + (c1 * e)
    bc_fill(out, bcs)
    return out


def march(phi: Tensor, u, nu, dt: float, nsteps: int, mesh, bcs: Sequence, limiter="upwind", order: int = 3, S=None,
          self_adv: bool = False, step=euler_step) -> Tensor:
    """``nsteps`` SSP Runge-Kutta steps of ``order`` (1: Euler) with the frozen source S; self_adv: every Euler step / stage is
    advected by its own input"""
    for _ in range(nsteps):
        phi0 = phi
        phi = step(phi0, phi0 if self_adv else u, nu, dt, mesh, bcs, limiter, *(() if S is None else (S,)))
        for c0, c1 in SSP_STAGES[order]:
            phi = rk_stage(phi, phi0, c0, c1, phi if self_adv else u, nu, dt, mesh, bcs, limiter, S, step)
    return phi


def fixed_point_source(phi: Tensor, u, nu, mesh, bcs: Sequence, limiter="upwind") -> Tensor:
    """S = -(nu * lap - adv) of ``phi`` with the step's own rounded operations, at every node (1, *n): with it ``a + s`` of
    E_S(phi) is an exact zero on the interior set, so a BC-filled ``phi`` is a fixed point of the step, bit for bit"""
    a = diffusion(phi, nu, mesh, bcs)
    a = a - advection(phi, u, mesh, bcs, limiter)
    return -a


# ---- momentum -------------------------------------------------------------------------------------------------------
class momentum:
    """The march of a vector field V (d, *n) that advects itself.  ``bcs`` is a list of d oracle BC lists: one BC type per
    face for all components, the face values per component.  ``nu`` a number, or one diffusivity field for every component.
    ``S`` is None or d entries (None, a number or a tensor each); ``u`` a frozen velocity instead of the input (the
    linearised form: d scalar marches)."""

    @staticmethod
    def _vel(V: Tensor, u: Sequence | None) -> list:
        return [V[a] for a in range(V.shape[0])] if u is None else list(u)

    @staticmethod
    def euler_step(V: Tensor, nu, dt: float, mesh, bcs: Sequence[Sequence], limiter="upwind", S: Sequence | None = None,
                   u: Sequence | None = None) -> Tensor:
        """E(V): every component stepped from the same input vector"""
        d = V.shape[0]
        assert d == mesh.dim and len(bcs) == d and (S is None or len(S) == d)
        vel = momentum._vel(V, u)
        return torch.cat([euler_step(V[c:c + 1], vel, nu, dt, mesh, bcs[c], limiter, None if S is None else S[c])
                          for c in range(d)])

    @staticmethod
    def rk_stage(V: Tensor, V0: Tensor, c0: float, c1: float, nu, dt: float, mesh, bcs: Sequence[Sequence],
                 limiter="upwind", S: Sequence | None = None, u: Sequence | None = None) -> Tensor:
        """B_c(c0 V0_c + c1 E(V)_c) for every component"""
        vel = momentum._vel(V, u)
        return torch.cat([rk_stage(V[c:c + 1], V0[c:c + 1], c0, c1, vel, nu, dt, mesh, bcs[c], limiter,
                                   None if S is None else S[c]) for c in range(V.shape[0])])

    @staticmethod
    def march(U: Tensor, nu, dt: float, nsteps: int, mesh, bcs: Sequence[Sequence], limiter="upwind", order: int = 3,
              S: Sequence | None = None, u: Sequence | None = None) -> Tensor:
        """``nsteps`` SSP Runge-Kutta steps of ``order``; every stage is advected by ITS OWN input (or by the frozen ``u``)"""
        for _ in range(nsteps):
            U0 = U
            U = momentum.euler_step(U0, nu, dt, mesh, bcs, limiter, S, u)
            for c0, c1 in SSP_STAGES[order]:
                U = momentum.rk_stage(U, U0, c0, c1, nu, dt, mesh, bcs, limiter, S, u)
        return U
