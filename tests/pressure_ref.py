"""The pressure-carrying projection step and the flow diagnostics restated on the CPU in torch, operation for operation what
``k_project_update`` and ``k_flow_stats`` compute (include/pyapes_hip.h "incremental projection and flow diagnostics", DESIGN.md
section 4 "Incremental form" / "Flow diagnostics"), and ``ns_step(form=...)`` built from tests/projection_ref.py,
``march_ref.momentum`` and the oracle's CG.  A plain module, no test lives here: the yardstick of tests/test_pressure_host.py
and tests/test_gpu_pressure.py.

Every operation is rounded on its own in the field's dtype; the scalars (scale, chi, q_a = 1 / dx_a) are formed in double and
converted once:
    update       U_c = U_c - scale * d_c phi on the interior set (projection_ref.correct), then B(U);  at EVERY node
                 q = p + phi;  nrhs given: t = chi * nrhs; q = q + t;  p = q
    flow_stats   rate    = max over all nodes of s,  r = |U_a| * q_a; s = s + r  (s starts at +0, axes ascending)
                 div_max = max over the interior set of |s|, s the restated divergence (scale 1: 1 * s is s)
                 div_sq  = sum over the interior set of (double)(s * s);   ke_sq = sum over all nodes and axes of (double)(U_a * U_a)
A NaN in a contribution makes a maximum NaN (``torch.max`` propagates it).  The sums here are ``math.fsum``: the correctly
rounded sum, which a sum of the same N non-negative doubles in ANY order meets within 2 N 2^-53 relative
(tests/test_pressure_host.py).
"""
from __future__ import annotations

import math
import warnings
from typing import Sequence

import torch
from torch import Tensor

import march_ref as R
import projection_ref as PR
from pyapes_oracle import OBC, bc_fill, interior_slicer, make_bcs, solve_poisson

FORMS = ("chorin", "incremental", "rotational")
SUM_BOUND = 2.0 ** -52          # times N: 2 N 2^-53, a sum of N non-negative doubles in any order against the exact one


def in_dtype(v: float, dtype: torch.dtype) -> Tensor:
    """a scalar formed in double, converted once"""
    return torch.tensor(float(v), dtype=torch.float64).to(dtype)


def update(U: Tensor, phi: Tensor, p: Tensor, nrhs: Tensor | None, scale: float, chi: float, mesh, ubcs: Sequence,
           fill: bool = True) -> tuple[Tensor, Tensor]:
    """(U, p) after ``pa_project_update``: ``U`` (d, *n), ``phi`` / ``p`` / ``nrhs`` (1, *n), phi BC-filled; the inputs stay"""
    assert phi.shape == p.shape and phi.shape[0] == 1 and (nrhs is None or nrhs.shape == p.shape)
    Un = PR.correct(U, phi, mesh, ubcs, scale, fill=fill)
    q = p + phi
    if nrhs is not None:
        t = in_dtype(chi, p.dtype) * nrhs
        q = q + t
    return Un, q


def inverse_spacing(mesh, dtype: torch.dtype) -> list[Tensor]:
    """q_a = fl(1 / dx_a): the quotient in double, converted to the dtype once"""
    return [in_dtype(1.0 / float(mesh.dx[a]), dtype) for a in range(mesh.dim)]


def rate_field(U: Tensor, mesh) -> Tensor:
    """s of ``rate`` at every node"""
    q = inverse_spacing(mesh, U.dtype)
    s = torch.zeros_like(U[0])
    for a in range(mesh.dim):
        r = U[a].abs() * q[a]
        s = s + r
    return s


def flow_stats(U: Tensor, mesh, bcs: Sequence) -> dict:
    """the four numbers of ``pa_flow_stats`` of the BC-filled vector ``U`` (d, *n), as Python floats"""
    assert U.shape[0] == mesh.dim and mesh.dim >= 2
    sl = interior_slicer(mesh.dim, bcs)
    d = PR.divergence(U, mesh, bcs, 1.0)[0][sl]
    return {"rate": float(rate_field(U, mesh).double().max()),
            "div_max": float(d.abs().double().max()),
            "div_sq": math.fsum((d * d).double().flatten().tolist()),
            "ke_sq": math.fsum(v for a in range(mesh.dim) for v in (U[a] * U[a]).double().flatten().tolist())}


def addends(U: Tensor, mesh, bcs: Sequence) -> tuple[int, int]:
    """how many doubles ``div_sq`` and ``ke_sq`` add up"""
    return PR.divergence(U, mesh, bcs)[0][interior_slicer(mesh.dim, bcs)].numel(), U.numel()


def component_bcs(ubcs: Sequence, d: int) -> list[list]:
    """one oracle BC list per component (what ``march_ref.momentum`` takes) from the list whose values hold one per component"""
    return [[OBC(b.face, b.type, b.val[c] if isinstance(b.val, list) else b.val, b.mesh, b.opt) for b in ubcs] for c in range(d)]


def increment_cfg(pcfg: Sequence[dict]) -> list[dict]:
    """the homogeneous counterpart of ``p``'s BC config: every value 0.0, a face without one (periodic) keeps None"""
    return [dict(c, bc_val=None if c["bc_val"] is None else 0.0) for c in pcfg]


def _cg(mesh, cfg, nrhs: Tensor, x0: Tensor, tol: float, max_it: int):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, rep = solve_poisson(mesh, cfg, nrhs, x0=x0, method="cg", tol=tol, max_it=max_it, coeff=1.0, sign=-1.0)
    return bc_fill(x.clone(), make_bcs(mesh, cfg)), rep


def ns_step(U: Tensor, p: Tensor, nu: float, dt: float, rho: float, mesh, ubcs: Sequence, pcfg: Sequence[dict], form: str,
            tol: float, max_it: int, limiter: str = "upwind", order: int = 3, S: Tensor | None = None) -> tuple[Tensor, Tensor, dict]:
    """One step on the CPU.  "chorin": the momentum step, then projection_ref.project.  "incremental" / "rotational": exactly
    the seven statements of pyapes_amd/solver/projection.py.  ``S``: None or a (d, *n) tensor.  Returns (U, p, report); the
    inputs stay."""
    assert form in FORMS
    d = mesh.dim
    cb = component_bcs(ubcs, d)
    if form == "chorin":
        Us = R.momentum.march(U, nu, dt, 1, mesh, cb, limiter, order, None if S is None else [S[c] for c in range(d)])
        return PR.project(Us, p, dt, rho, mesh, ubcs, pcfg, tol, max_it)
    pbcs = make_bcs(mesh, pcfg)
    p = bc_fill(p.clone(), pbcs)                                                            # 1
    src = PR.correct(torch.zeros_like(U) if S is None else S, p, mesh, ubcs, 1.0 / rho, fill=False)   # 2
    Us = R.momentum.march(U, nu, dt, 1, mesh, cb, limiter, order, [src[c] for c in range(d)])         # 3
    Us = bc_fill(Us.clone(), ubcs)
    nrhs = PR.divergence(Us, mesh, ubcs, -(rho / dt))                                       # 4
    phi, rep = _cg(mesh, increment_cfg(pcfg), nrhs, torch.zeros_like(p), tol, max_it)       # 5
    Un, q = update(Us, phi, p, nrhs if form == "rotational" else None, dt / rho, nu * dt, mesh, ubcs)   # 6
    return Un, bc_fill(q, pbcs), rep                                                        # 7


# ---- the fluid at rest under a body force (DESIGN.md section 4 "Incremental form", the table) -----------------------
REST_NU, REST_DT, REST_RHO, REST_STEPS = 1e-2, 5e-3, 1.3, 3


def rest_case(n: Sequence[int], dtype: str):
    """(oracle mesh, ubcs, U's face values and types, pcfg, U = 0, the BC-filled p0, S) on the unit box: walls on U;
    p0 = cos(pi x / 2) cos(pi y) [cos(pi z)] with p Neumann 0 on every face but xu, Dirichlet 0 there; S_c the restated
    (1 / rho) grad_c(p0) on the interior set, 0 off it: the body force that p0 balances"""
    from pyapes_oracle import FACES, OMesh, mixed_cfg
    nd = len(n)
    om = OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
    utypes, uvals = ["dirichlet"] * (2 * nd), [[0.0] * nd for _ in range(2 * nd)]
    ptypes = ["neumann", "dirichlet"] + ["neumann"] * (2 * nd - 2)
    ubcs = make_bcs(om, mixed_cfg(uvals, utypes, FACES[:2 * nd]))
    pcfg = mixed_cfg([0.0] * (2 * nd), ptypes, FACES[:2 * nd])
    X = [g.double() for g in om.grid]
    p0 = torch.cos(0.5 * math.pi * X[0])
    for a in range(1, nd):
        p0 = p0 * torch.cos(math.pi * X[a])
    p0 = bc_fill(p0.to(om.dtype).unsqueeze(0), make_bcs(om, pcfg))
    U0 = torch.zeros((nd, *n), dtype=om.dtype)
    S = -PR.correct(U0, p0, om, ubcs, 1.0 / REST_RHO, fill=False)
    S = S + torch.zeros_like(S)            # -0 off the interior set -> +0
    return om, ubcs, (uvals, utypes), (pcfg, ptypes), U0, p0, S
