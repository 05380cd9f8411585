"""The projection layer restated on the CPU in torch, operation for operation what ``k_divergence``, ``k_project_correct``,
``k_project_update`` and ``k_flow_stats`` compute (include/pyapes_hip.h "projection" and "incremental projection and flow
diagnostics", DESIGN.md section 4 "Projection" / "Incremental form" / "Flow diagnostics"), and the steps built from them,
``march_ref.momentum`` and the oracle's CG: ``project`` and ``ns_step(form=...)``.  A plain module, no test lives here: the
yardstick of tests/test_projection_host.py, tests/test_pressure_host.py, tests/test_gpu_projection.py and
tests/test_gpu_pressure.py, as march_ref.py is the marches'.

Per mesh axis a, every operation rounded on its own in the field's dtype, the scalars (scale, chi, h_a = 0.5 / dx_a,
q_a = 1 / dx_a, dx_a the spacing as the mesh dtype stores it) formed in double and converted once (``in_dtype``), neighbours
wrapping around (``torch.roll``):
    divergence   d = U_a[+1]_a - U_a[-1]_a;  d = d * h_a;  s = s + d   (s starts at +0, axes ascending);   out = scale * s
    correction   g = p[+1]_c - p[-1]_c;  g = g * h_c;  g = scale * g;  out_c = U_c - g
    update       the correction with phi for p, then B(U);  at EVERY node
                 q = p + phi;  nrhs given: t = chi * nrhs; q = q + t;  p = q
    flow_stats   rate    = max over all nodes of s,  r = |U_a| * q_a; s = s + r  (s starts at +0, axes ascending)
                 div_max = max over the interior set of |s|, s the restated divergence (scale 1: 1 * s is s)
                 div_sq  = sum over the interior set of (double)(s * s);   ke_sq = sum over all nodes and axes of (double)(U_a * U_a)
on the interior set of the BC list (the oracle's ``interior_slicer``: [1:-1] per axis, an end opened by a periodic face); off
it the divergence is +0 and the correction hands U_c on.  All read BC-filled inputs: the caller fills them.  A NaN in a
contribution makes a maximum NaN (``torch.max`` propagates it).  The sums here are ``math.fsum``: the correctly rounded sum,
which a sum of the same N non-negative doubles in ANY order meets within 2 N 2^-53 relative (tests/test_pressure_host.py).
"""
from __future__ import annotations

import math
import warnings
from typing import Sequence

import numpy as np
import torch
from torch import Tensor

import march_ref as R
from pyapes_oracle import FACES_RZ, OBC, bc_fill, interior_slicer, solve_poisson, make_bcs

FORMS = ("chorin", "incremental", "rotational")
SUM_BOUND = 2.0 ** -52          # times N: 2 N 2^-53, a sum of N non-negative doubles in any order against the exact one


def in_dtype(v: float, dtype: torch.dtype) -> Tensor:
    """a scalar formed in double, converted once"""
    return torch.tensor(float(v), dtype=torch.float64).to(dtype)


# ---- the walled single-mode problem (tests/test_projection_host.py derives what the projection leaves of it) ---------------
MODE_N, MODE_M = 17, 4           # the phase advances by theta = MODE_M pi / (MODE_N - 1) = pi / 4 per node on both axes
MODE_DT, MODE_RHO = 0.01, 1.3
# sin^2(theta / 2) at theta = pi / 4 (tests/test_projection_host.py derives it): the fraction of the mode's divergence that the
# approximate projection leaves
REMAINING_FRACTION = (2.0 - math.sqrt(2.0)) / 4.0


def mode_case(dtype: str):
    """(oracle mesh, U, the Dirichlet values of U per face and component): on the unit square, U = (cos sin, 1/2 sin cos) of
    the sine mode sin(theta i) sin(theta j), whose divergence is that mode on the interior set; the faces of U hold the mode's
    own values, p is 0 on every face"""
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
    return [in_dtype(0.5 / float(mesh.dx[a]), dtype) for a in range(mesh.dim)]


def divergence(U: Tensor, mesh, bcs: Sequence, scale: float = 1.0) -> Tensor:
    """(1, *n): ``scale`` times the central divergence of the BC-filled vector ``U`` (d, *n) on the interior set of ``bcs``"""
    assert U.shape[0] == mesh.dim and mesh.dim >= 2
    h = half_inverse_spacing(mesh, U.dtype)
    sc = in_dtype(scale, U.dtype)
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
    sc = in_dtype(scale, U.dtype)
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


def cg(mesh, cfg: Sequence[dict], nrhs: Tensor, x0: Tensor, tol: float, max_it: int) -> tuple[Tensor, dict]:
    """the oracle's CG on -lap(x) = nrhs with the BCs of config ``cfg`` from ``x0``, then B(x): (x, report)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, rep = solve_poisson(mesh, cfg, nrhs, x0=x0, method="cg", tol=tol, max_it=max_it, coeff=1.0, sign=-1.0)
    return bc_fill(x.clone(), make_bcs(mesh, cfg)), rep


def project(U: Tensor, p: Tensor, dt: float, rho: float, mesh, ubcs: Sequence, pcfg: Sequence[dict], tol: float,
            max_it: int) -> tuple[Tensor, Tensor, dict]:
    """The projection step on the CPU: B(U); -rhs = -(rho / dt) div(U); the oracle's CG on -lap(p) = -rhs with ``p``'s BCs
    (config ``pcfg``) from ``p``'s content; B(p); U <- B(U - (dt / rho) grad(p)).  Returns (U, p, report); the inputs stay."""
    U = bc_fill(U.clone(), ubcs)
    x, rep = cg(mesh, pcfg, divergence(U, mesh, ubcs, -(rho / dt)), p.clone(), tol, max_it)
    return correct(U, x, mesh, ubcs, dt / rho), x, rep


# ---- the pressure-carrying forms and the flow diagnostics --------------------------------------------------------------
def update(U: Tensor, phi: Tensor, p: Tensor, nrhs: Tensor | None, scale: float, chi: float, mesh, ubcs: Sequence,
           fill: bool = True) -> tuple[Tensor, Tensor]:
    """(U, p) after ``pa_project_update``: ``U`` (d, *n), ``phi`` / ``p`` / ``nrhs`` (1, *n), phi BC-filled; the inputs stay"""
    assert phi.shape == p.shape and phi.shape[0] == 1 and (nrhs is None or nrhs.shape == p.shape)
    Un = correct(U, phi, mesh, ubcs, scale, fill=fill)
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
    d = divergence(U, mesh, bcs, 1.0)[0][sl]
    return {"rate": float(rate_field(U, mesh).double().max()),
            "div_max": float(d.abs().double().max()),
            "div_sq": math.fsum((d * d).double().flatten().tolist()),
            "ke_sq": math.fsum(v for a in range(mesh.dim) for v in (U[a] * U[a]).double().flatten().tolist())}


def addends(U: Tensor, mesh, bcs: Sequence) -> tuple[int, int]:
    """how many doubles ``div_sq`` and ``ke_sq`` add up"""
    return divergence(U, mesh, bcs)[0][interior_slicer(mesh.dim, bcs)].numel(), U.numel()


def component_bcs(ubcs: Sequence, d: int) -> list[list]:
    """one oracle BC list per component (what ``march_ref.momentum`` takes) from the list whose values hold one per component"""
    return [[OBC(b.face, b.type, b.val[c] if isinstance(b.val, list) else b.val, b.mesh, b.opt) for b in ubcs] for c in range(d)]


def increment_cfg(pcfg: Sequence[dict]) -> list[dict]:
    """the homogeneous counterpart of ``p``'s BC config: every value 0.0, a face without one (periodic) keeps None"""
    return [dict(c, bc_val=None if c["bc_val"] is None else 0.0) for c in pcfg]


def ns_step(U: Tensor, p: Tensor, nu: float, dt: float, rho: float, mesh, ubcs: Sequence, pcfg: Sequence[dict], form: str,
            tol: float, max_it: int, limiter: str = "upwind", order: int = 3, S: Tensor | None = None) -> tuple[Tensor, Tensor, dict]:
    """One step on the CPU.  "chorin": the momentum step, then ``project``.  "incremental" / "rotational": exactly
    the seven statements of pyapes_amd/solver/projection.py.  ``S``: None or a (d, *n) tensor.  Returns (U, p, report); the
    inputs stay."""
    assert form in FORMS
    d = mesh.dim
    cb = component_bcs(ubcs, d)
    if form == "chorin":
        Us = R.momentum.march(U, nu, dt, 1, mesh, cb, limiter, order, None if S is None else [S[c] for c in range(d)])
        return project(Us, p, dt, rho, mesh, ubcs, pcfg, tol, max_it)
    pbcs = make_bcs(mesh, pcfg)
    p = bc_fill(p.clone(), pbcs)                                                            # 1
    src = correct(torch.zeros_like(U) if S is None else S, p, mesh, ubcs, 1.0 / rho, fill=False)   # 2
    Us = R.momentum.march(U, nu, dt, 1, mesh, cb, limiter, order, [src[c] for c in range(d)])         # 3
    Us = bc_fill(Us.clone(), ubcs)
    nrhs = divergence(Us, mesh, ubcs, -(rho / dt))                                          # 4
    phi, rep = cg(mesh, increment_cfg(pcfg), nrhs, torch.zeros_like(p), tol, max_it)        # 5
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
    S = -correct(U0, p0, om, ubcs, 1.0 / REST_RHO, fill=False)
    S = S + torch.zeros_like(S)            # -0 off the interior set -> +0
    return om, ubcs, (uvals, utypes), (pcfg, ptypes), U0, p0, S


# ---- what the two host test modules share -----------------------------------------------------------------------------
def eps_of(dtype):
    return float(torch.finfo(dtype).eps)


MIXED_TYPES = ["dirichlet", "neumann", "symmetry", "dirichlet", "periodic", "periodic"]


def smooth_vector(om):
    """a smooth vector field with distinct components and a smooth scalar, float64 numpy, on the mesh's nodes"""
    X = [g.double().numpy() for g in om.grid]
    nd = om.dim
    U = np.stack([np.sin(1.3 * X[a] + 0.4 * a) * np.cos(0.7 * X[(a + 1) % nd] - 0.2) + 0.1 * (a + 1) for a in range(nd)])
    p = np.cos(0.9 * X[0] + 0.3) * np.sin(1.1 * X[-1] + 0.5) + 0.25
    return U, p


def interior_mask(om, bcs):
    m = np.zeros(tuple(om.nx), dtype=bool)
    m[interior_slicer(om.dim, bcs)] = True
    return m


def cpu_field(n=(9, 9), dim=None, slab=None, geo=None, dtype="double", name="U", mesh=None):
    """a Field of the package on a CPU mesh, Dirichlet 0 on every face: what the argument checks are shown"""
    from pyapes_amd.geometry import Box
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.variables import Field
    from pyapes_amd.variables.bcs import mixed_bcs
    if mesh is None:
        box = geo if geo is not None else (Box[0:1] if len(n) == 1 else (Box[0:1, 0:1] if len(n) == 2 else Box[0:1, 0:1, 0:1]))
        mesh = Mesh(box, None, list(n), "cpu", dtype, **({"slab": slab} if slab else {}))
    nd = mesh.dim
    cfg = mixed_bcs([0.0] * (2 * nd), ["dirichlet"] * (2 * nd))
    if mesh.coord_sys == "rz":
        cfg = [dict(c, bc_face=f) for c, f in zip(cfg, FACES_RZ)]
    return Field(name, nd if dim is None else dim, mesh, {"domain": cfg, "obstacle": None})
