"""Shared builders for the parity tests: the same case descriptors drive the oracle
(tests only) and the product path (pyapes_amd on the GPU through the C ABI)."""
from __future__ import annotations

import contextlib
import os

import numpy as np
import torch

import pyapes_oracle as O
from pyapes_amd.geometry import Box, Cylinder
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdm import FDM
from pyapes_amd.solver.ops import Solver
from pyapes_amd.testing.poisson import poisson_bcs
from pyapes_amd.variables import Field

FACES = O.FACES

HOSTRING_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libpa_hostring.so")


def hip_options(monkeypatch, **kw):
    """Options of every pa_ctx created from now on, in this process and in the processes it starts:
    PYAPES_HIP_OPTIONS="name=value,..." (pa_ctx_set_option names; None takes a name out again)."""
    cur = dict(item.split("=") for item in os.environ.get("PYAPES_HIP_OPTIONS", "").split(",") if item)
    for k, v in kw.items():
        if v is None:
            cur.pop(k, None)
        else:
            cur[k] = str(int(v))
    if cur:
        monkeypatch.setenv("PYAPES_HIP_OPTIONS", ",".join(f"{k}={v}" for k, v in cur.items()))
    else:
        monkeypatch.delenv("PYAPES_HIP_OPTIONS", raising=False)


def use_hostring():
    """Hand the test stand-in for librccl (tests/lib/pa_hostring.hip: ranks as processes that may share one GPU, host
    shared memory as the wire) to libpyapes_hip -- an explicit call in every rank process, before its first communicator."""
    from pyapes_amd.hip.lib import load_library
    assert os.path.exists(HOSTRING_LIB), f"{HOSTRING_LIB} missing: pyapes_amd/csrc/build.sh builds it"
    rc = load_library().pa_comm_use_impl(HOSTRING_LIB.encode())
    assert rc == 0, f"pa_comm_use_impl({HOSTRING_LIB}) -> {rc}"


def case_faces(case):
    return O.FACES_RZ if case.get("coord", "xyz") == "rz" else FACES


def oracle_cfg(case):
    nd = len(case["lower"])
    if case["bcs"] == "poisson":
        return O.poisson_cfg(nd)
    if case["bcs"] == "poisson_rz":
        return O.poisson_rz_cfg()
    if case["bcs"] == "robin":
        return O.robin_cfg(nd)
    faces = case_faces(case)
    return [{"bc_face": faces[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(case["bcs"])]


def product_cfg(case):
    nd = len(case["lower"])
    if case["bcs"] == "poisson":
        return poisson_bcs(nd)
    if case["bcs"] == "poisson_rz":
        from pyapes_amd.testing.poisson import poisson_rz_bcs
        return poisson_rz_bcs()
    if case["bcs"] == "robin":   # callables that READ THE FIELD (the same functions drive reference, oracle and product)
        return [dict(d, bc_val_opt=None) for d in O.robin_cfg(nd)]
    faces = case_faces(case)
    return [{"bc_face": faces[i], "bc_type": t, "bc_val": v, "bc_val_opt": None}
            for i, (t, v) in enumerate(case["bcs"])]


def oracle_mesh(case):
    return O.OMesh(case["lower"], case["upper"], case["spacing"], case["dtype"], case.get("coord", "xyz"))


def product_mesh(case, device="cuda"):
    geo = Cylinder if case.get("coord", "xyz") == "rz" else Box
    return Mesh(geo(case["lower"], case["upper"]), None, case["spacing"], device, case["dtype"])


def product_field(case, mesh, x0=None):
    var = Field("p", 1, mesh, {"domain": product_cfg(case), "obstacle": None})
    if x0 is not None:
        var.set_var_tensor(torch.as_tensor(x0).to(mesh.device).clone())
    return var


def product_solve(case, rhs0, K, method=None, x0=None):
    """rhs0: numpy/tensor (1,*nx).  Returns (x cpu tensor, report, solver)."""
    mesh = product_mesh(case)
    var = product_field(case, mesh, x0)
    rhs = torch.as_tensor(rhs0).to(mesh.device).clone()
    solver = Solver({"fdm": {"method": method or case["method"], "tol": case["tol"], "max_it": K,
                             "report": False}})
    fdm = FDM()
    coeff, sign = case.get("coeff", 1.0), case.get("sign", 1.0)
    eq = fdm.laplacian(coeff, var) if sign > 0 else -fdm.laplacian(coeff, var)
    solver.set_eq(eq == rhs)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rep = solver.solve()
    return var().cpu(), rep, solver


def rel_err(a, b):
    a = torch.as_tensor(a).double()
    b = torch.as_tensor(b).double()
    return float(torch.linalg.norm(a - b)) / max(float(torch.linalg.norm(b)), 1e-300)


def bit_equal(a, b):
    return torch.equal(torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu())


_BITS = {torch.float32: torch.int32, torch.float64: torch.int64}


class _Bits:
    """the verdict of ``same_bits``: true or false, and on failure its ``why`` names the first cell that differs"""

    def __init__(self, ok, why=""):
        self.ok, self.why = bool(ok), why

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return "same bits" if self.ok else self.why


def same_bits(a, b):
    """``a`` and ``b`` (fp32 or fp64, equal dtypes and shapes) hold the same BITS: the NaN masks are equal -- a NaN is a
    class, its sign and payload are not compared -- and every other element has the same integer view (int32 / int64), so
    -0 is not +0 and a subnormal is not 0.  False comes with the first differing index and both bit patterns (``.why``,
    which is also its repr: ``assert same_bits(a, b)`` reports it)."""
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    if a.dtype != b.dtype or a.dtype not in _BITS:
        return _Bits(False, "dtypes %s / %s: fp32 or fp64 on both sides" % (a.dtype, b.dtype))
    if a.shape != b.shape:
        return _Bits(False, "shapes %s / %s" % (tuple(a.shape), tuple(b.shape)))
    na, nb = torch.isnan(a), torch.isnan(b)
    ia, ib = a.view(_BITS[a.dtype]), b.view(_BITS[a.dtype])
    bad = (na != nb) | (~na & ~nb & (ia != ib))
    if not bool(bad.any()):
        return _Bits(True)
    flat = int(bad.flatten().nonzero()[0])
    idx = tuple(int(i) for i in np.unravel_index(flat, tuple(a.shape))) if a.dim() else ()
    mask = (1 << (8 * a.element_size())) - 1
    va, vb = a.flatten()[flat], b.flatten()[flat]
    pa, pb = int(ia.flatten()[flat]) & mask, int(ib.flatten()[flat]) & mask
    width = 2 * a.element_size()
    return _Bits(False, "%d of %d cells differ; the first at %s: %r (0x%0*X) / %r (0x%0*X)"
                 % (int(bad.sum()), a.numel(), idx, float(va), width, pa, float(vb), width, pb))


GUARD_SENTINEL = -123456.789   # finite, and no input of the tests holds it (fields are rand / randn / small BC values)


def offset_view(t, k, guard=16):
    """``t`` as an operand that is NOT 16-byte aligned: a contiguous view of ``t``'s shape, holding ``t``'s values, that
    starts ``k`` elements past a 16-byte boundary inside a fresh allocation (same dtype and device) with at least ``guard``
    elements in front of it and behind it, all GUARD_SENTINEL.  ``k`` = 0 gives an aligned view with the same guards.
    Returns (view, allocation).  Every access a kernel makes to the view, of any width, stays inside the allocation; a
    store outside the array shows up as a changed guard (``guards_intact``)."""
    t = torch.as_tensor(t)
    n = t.numel()
    guard, k = max(int(guard), 1), int(k)
    alloc = torch.full((guard + 16 + k + n + guard + 16,), GUARD_SENTINEL, dtype=t.dtype, device=t.device)
    es = alloc.element_size()
    # the first 16-byte boundary at least `guard` elements in (device allocations start on one; a host one need not)
    front = guard + (-(alloc.data_ptr() // es + guard)) % max(16 // es, 1) + k
    view = alloc[front:front + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == alloc.data_ptr() + front * es
    assert view.data_ptr() % 16 == (k * es) % 16
    return view, alloc


def guards_intact(alloc, view):
    """True when every element of ``alloc`` outside ``view`` still holds GUARD_SENTINEL, bit for bit."""
    es = alloc.element_size()
    front = (view.data_ptr() - alloc.data_ptr()) // es
    bits = {8: torch.int64, 4: torch.int32, 2: torch.int16}[es]
    a = alloc.view(bits)
    want = torch.full((1,), GUARD_SENTINEL, dtype=alloc.dtype, device=alloc.device).view(bits)
    lo, hi = a[:front], a[front + view.numel():]
    return lo.numel() > 0 and hi.numel() > 0 and bool((lo == want).all()) and bool((hi == want).all())


class SumTap:
    """Records the value of every ``torch.sum(t, dim=...)`` made while it is active -- the dot products of the
    reference's (and the oracle's) solver loops (linalg.py:119-137, 204-250), which is all they use it for.
    It wraps whatever ``torch.sum`` is at that moment, so it goes on LAST (outside a reordering ``fsum``)."""

    def __init__(self):
        self.vals = []

    def __enter__(self):
        self.prev = torch.sum
        prev, vals = self.prev, self.vals

        def tap(t, dim=None, **kw):
            if dim is None:
                return prev(t, **kw)
            r = prev(t, dim=dim, **kw)
            vals.append(float(r.reshape(-1)[0]))
            return r

        torch.sum = tap
        return self

    def __exit__(self, *exc):
        torch.sum = self.prev


def scalar_history(method, sums):
    """The per-iteration scalars the solver loops compute from their dot products and drop, rebuilt from the
    recorded sums: CG -> rows (alpha, beta) from (r.r, d.Ad, r.r, r'.r') per iteration (linalg.py:118-137);
    BiCGSTAB -> rows (alpha, omega, rho_next) from r0.r0, then (r0.v [, t.s, t.t, r0.t]) per iteration
    (linalg.py:204-250; the iteration that leaves through the first stop test has alpha only)."""
    def nn(v):
        return 0.0 if (v != v or v in (float("inf"), float("-inf"))) else v
    rows = []
    if method == "cg":
        for i in range(len(sums) // 4):
            rr, dad, rr2, rrn = sums[4 * i:4 * i + 4]
            rows.append((nn(rr / dad) if dad != 0 else 0.0, rrn / rr2 if rr2 != 0 else float("nan")))
        return np.array(rows, dtype=np.float64).reshape(-1, 2)
    rho, i = sums[0], 1
    while i < len(sums):
        alpha = nn(rho / sums[i]) if sums[i] != 0 else 0.0
        if i + 3 <= len(sums) - 1:
            ts, tt, r0t = sums[i + 1:i + 4]
            omega = nn(ts / tt) if tt != 0 else 0.0
            rho = -omega * r0t
            rows.append((alpha, omega, rho))
            i += 4
        else:
            rows.append((alpha, float("nan"), float("nan")))
            i += 1
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


@contextlib.contextmanager
def sum_order(variant):
    """While active, every ``torch.sum`` is evaluated in a different, equally valid order (variant 1 / 2 / 3:
    reversed along all / the first / the last summed axis; 4: as two half sums; 0: torch's own)."""
    orig = torch.sum

    def fsum(t, dim=None, **kw):
        dims = tuple(range(t.dim())) if dim is None else tuple(dim)
        if variant == 4:
            if dim is None:
                f = t.contiguous().flatten()
                h = f.numel() // 2
                return orig(f[:h]) + orig(f[h:])
            f = t.contiguous().flatten(1)
            h = f.shape[1] // 2
            return orig(f[:, :h], dim=1) + orig(f[:, h:], dim=1)
        fd = {1: dims, 2: dims[:1], 3: dims[-1:]}[variant]
        tt = t.flip(fd).contiguous()
        return orig(tt) if dim is None else orig(tt, dim=dim)

    if variant:
        torch.sum = fsum
    try:
        yield
    finally:
        torch.sum = orig


# ---- multi-term equations (golden kind "eqn", tests/test_gpu_equations.py) ----
def eqn_tensor(case, shape, dtype):
    """The tensor parameter of an equation case: a Div speed (randn, both signs) or a Laplacian coefficient (> 0)."""
    g = torch.Generator().manual_seed(case.get("seed", 0) + 7)
    t = torch.randn(shape, generator=g, dtype=torch.float64)
    if case.get("tensor", "randn") == "gamma":
        t = 0.2 + 0.1 * t.abs()
    return t.to(dtype)


def eqn_cfg(case):
    """Oracle BC list of an equation case: [type, value] pairs in face order, or a named set of callables."""
    if case["bcs"] == "pernode3d":
        return O.pernode_cfg()
    faces = case_faces(case)
    return [{"bc_face": faces[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(case["bcs"])]


def eqn_spec(case, tensor):
    """``O.equation_terms`` spec of ``case["terms"]`` = [kind, sign, parameter] per operator (parameter: a number, None,
    or "tensor" for the case's tensor) -- the equation that is SOLVED, which for an operator object used twice
    is not the one written (``case["dsl"]``)."""
    spec = []
    for kind, sign, p in case["terms"]:
        p = tensor if p == "tensor" else p
        if kind == "div":
            spec.append({"kind": "div", "sign": sign, "u": p, "limiter": case["limiter"]})
        else:
            spec.append({"kind": kind, "sign": sign, "coeff": p})
    return spec


def eqn_build(fdm, var, case, tensor):
    """The DSL expression of ``case["dsl"]`` (default: ``case["terms"]``), operator by operator in Python's evaluation
    order of ``[-]A +- B +- ...``, on the reference's FDM or the product's (same DSL).  ``tensor`` on var's device."""
    expr = None
    for kind, sign, p in case.get("dsl", case["terms"]):
        p = tensor if p == "tensor" else p
        op = getattr(fdm, kind)
        term = op(var) if p is None else op(p, var)
        if expr is None:
            expr = -term if sign < 0 else term
        else:
            expr = expr - term if sign < 0 else expr + term
    return expr


def eqn_inputs(case):
    """(x0, rhs0, tensor) of an equation case that has no fixture: the seeded recipe of tests/golden/make_golden.py"""
    dt = torch.float64 if case["dtype"] == "double" else torch.float32
    shape = (1, *case["spacing"])
    g = torch.Generator().manual_seed(case.get("seed", 0))
    rhs0 = torch.randn(shape, generator=g, dtype=torch.float64).to(dt)
    g = torch.Generator().manual_seed(case.get("seed", 0) + 100)
    x0 = torch.randn(shape, generator=g, dtype=torch.float64).to(dt)
    return x0, rhs0, eqn_tensor(case, shape, dt)


def eqn_oracle(case, x0, rhs0, tensor, K, variant=0):
    """The oracle on an equation case -> (rhs after set_eq, A x on the BC-filled x0, iterate, report); variant as in
    ``sum_order``."""
    import warnings
    mesh, cfg, spec = oracle_mesh(case), eqn_cfg(case), eqn_spec(case, tensor)
    bcs = O.make_bcs(mesh, cfg)
    xf = x0.clone()
    O.bc_fill(xf, bcs)
    ax = O.Aop(xf, O.equation_terms(mesh, bcs, spec, xf)[0], mesh.dim)
    rhs = rhs0.clone()
    with sum_order(variant), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        x, rep = O.solve_equation(mesh, cfg, spec, rhs, x0.clone(), case["method"], case["tol"], K)
    return rhs, ax, x, rep


# The two-term tiling of the 3-D / 2-D kernels needs whole rows and more than one k tile: meshes too large for
# fixtures, graded against the oracle (which the "eqn" goldens pin to the reference).  Shapes and face sets of
# tests/test_gpu_tiled_advdiff.py; BiCGSTAB, 3 iterations from a random x0.
_D, _N = (lambda v=0.0: ["dirichlet", v]), (lambda v=0.0: ["neumann", v])
_SY, _PE = ["symmetry", None], ["periodic", None]
TILED_EQN_BCS = {"mix": [_D(0.0), _N(0.5), _SY, _D(0.0), _D(1.0), _N(-0.25)],
                 "zper": [_D(0.5), _D(0.1), _D(0.0), _D(0.0), _PE, _PE]}
TILED_EQN_SHAPES = [((20, 18, 132), "double"), ((9, 17, 129), "double"), ((40, 132), "double"), ((16, 20, 136), "single")]
TILED_EQN_K = 3


def tiled_eqn_cases():
    """face set x scheme (literal upwind on both sets, central where no face is neumann / symmetry) x speed (+-0.8,
    and a tensor on the first shape) x both term orders / signs of the Div"""
    cases = []
    for n, dtype in TILED_EQN_SHAPES:
        nd = len(n)
        for bc, lim in (("mix", "upwind"), ("zper", "upwind"), ("zper", "none")):
            for utag, u in (("up", 0.8), ("um", -0.8), ("ut", "tensor")):
                if u == "tensor" and n != TILED_EQN_SHAPES[0][0]:
                    continue
                for order, terms in (("div_first", [["div", 1.0, u], ["laplacian", -1.0, 0.05]]),
                                     ("lap_first", [["laplacian", -1.0, 0.05], ["div", -1.0, u]])):
                    name = "x".join(map(str, n)) + f"{dtype[0]}_{bc}_{lim}_{utag}_{order}"
                    cases.append(dict(name=name, kind="eqn", lower=[0.0] * nd, upper=[1.0] * nd, spacing=list(n),
                                      dtype=dtype, bcs=TILED_EQN_BCS[bc][:2 * nd], terms=terms, limiter=lim,
                                      method="bicgstab", tol=1e-30, max_its=[TILED_EQN_K]))
    return cases


def oracle_solve(case, rhs0, K, variant=0, tap=None):
    """The oracle on a golden case.  variant > 0 evaluates every torch.sum in a different, equally
    valid order (reversed along all / the first / the last summed axis, or as two half sums):
    same algorithm, same inputs, same arithmetic otherwise."""
    import warnings
    mesh = oracle_mesh(case)
    with sum_order(variant), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with (tap if tap is not None else contextlib.nullcontext()):
            return O.solve_poisson(mesh, oracle_cfg(case), torch.as_tensor(rhs0).clone(), method=case["method"],
                                   tol=case["tol"], max_it=K, coeff=case.get("coeff", 1.0),
                                   sign=case.get("sign", 1.0))


def summation_band(case, rhs0, K):
    """(max rel. deviation of the result, list of iteration counts) of the REFERENCE ALGORITHM over
    five summation orders of its dot products.  BiCGSTAB and CG on the reference's non-symmetric
    periodic operator amplify 1e-16 perturbations; no implementation with a different
    reduction tree can be expected to sit closer to the reference than this band."""
    x0, r0 = oracle_solve(case, rhs0, K, 0)
    dev, its = 0.0, [r0["itr"]]
    for v in (1, 2, 3, 4):
        x, r = oracle_solve(case, rhs0, K, v)
        dev = max(dev, rel_err(x, x0))
        its.append(r["itr"])
    return dev, its


def _oracle_solve_random_order(case, rhs0, K, seed, tap=None):
    """the oracle with every torch.sum evaluated over a random permutation of its addends, split into a
    random number of partial sums: one more equally valid summation order of the same algorithm"""
    import warnings
    orig = torch.sum
    gen = torch.Generator().manual_seed(1000 + seed)

    def fsum(t, dim=None, **kw):
        f = t.contiguous().flatten() if dim is None else t.contiguous().flatten(1)
        perm = torch.randperm(f.shape[-1], generator=gen)
        nb = int(torch.randint(2, 64, (1,), generator=gen))
        acc = None
        for c in f[..., perm].chunk(nb, dim=-1):
            s = orig(c, dim=-1)
            acc = s if acc is None else acc + s
        return acc

    torch.sum = fsum
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with (tap if tap is not None else contextlib.nullcontext()):
                return O.solve_poisson(oracle_mesh(case), oracle_cfg(case), torch.as_tensor(rhs0).clone(),
                                       method=case["method"], tol=case["tol"], max_it=K,
                                       coeff=case.get("coeff", 1.0), sign=case.get("sign", 1.0))
    finally:
        torch.sum = orig


def summation_hull(case, rhs0, K, x_ref, n_random=24, histories=None):
    """The REFERENCE ALGORITHM evaluated with 5 structured + ``n_random`` random summation orders of its
    dot products -> (band, diam, iteration counts): band = largest rel. distance of a sample from ``x_ref``
    (the reference's own result), diam = largest rel. distance between two samples.
    See test_solve_vs_reference for how they grade.  ``histories`` (a list) receives every sample's
    per-iteration scalars (``scalar_history``)."""
    xs, its = [], []
    for v in range(5):
        tap = SumTap() if histories is not None else None
        x, r = oracle_solve(case, rhs0, K, v, tap=tap)
        xs.append(x)
        its.append(r["itr"])
        if tap is not None:
            histories.append(scalar_history(case["method"], tap.vals))
    for s in range(n_random):
        tap = SumTap() if histories is not None else None
        x, r = _oracle_solve_random_order(case, rhs0, K, s, tap=tap)
        xs.append(x)
        its.append(r["itr"])
        if tap is not None:
            histories.append(scalar_history(case["method"], tap.vals))
    band = max(rel_err(x, x_ref) for x in xs)
    n = len(xs)
    diam = max(rel_err(xs[i], xs[j]) for i in range(n) for j in range(i + 1, n))
    return band, diam, its


def agreement_horizon(ref_hist, histories, rtol):
    """First iteration (0-based) at which some reordered run of the reference algorithm differs from the
    reference's recorded scalars by more than ``rtol`` (relative, any column); len(ref_hist) if none does."""
    n = len(ref_hist)
    for i in range(n):
        for h in histories:
            if i >= len(h):
                return i
            a, b = ref_hist[i], h[i]
            for u, v in zip(a, b):
                if u != u and v != v:
                    continue
                if not abs(u - v) <= rtol * max(abs(u), 1e-300):
                    return i
    return n


def true_residual(case, rhs0, x):
    """|| (b_adj - A x) ||_2 over the interior set, evaluated by the product's own operator."""
    from pyapes_amd.mesh.tools import boundary_slicer
    mesh = product_mesh(case)
    var = product_field(case, mesh, x)
    rhs = torch.as_tensor(rhs0).to(mesh.device).clone()
    solver = Solver({"fdm": {"method": "cg", "tol": 1e-6, "max_it": 1, "report": False}})
    fdm = FDM()
    coeff, sign = case.get("coeff", 1.0), case.get("sign", 1.0)
    eq = fdm.laplacian(coeff, var) if sign > 0 else -fdm.laplacian(coeff, var)
    solver.set_eq(eq == rhs)
    S = tuple(boundary_slicer(mesh.dim, var.bcs))
    r = (solver.rhs - solver.Aop(var))[0][S]
    return float(torch.linalg.norm(r))
