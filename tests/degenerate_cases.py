"""The solver loops where their scalars degenerate: the case table and its builders.  A plain module: no test lives here.
tests/test_degenerate_host.py proves on the CPU oracle what each family claims; tests/test_gpu_degenerate.py runs the
same cases through every solver path of the library and demands the oracle's bits.

    A  zero residual at the start (rhs = 0 on x0 = 0, or on x0 = 0.3 with Dirichlet 0.3): 0/0 -> 0, beta = 0/0 = NaN,
       `!(tol > tolerance)` with tol == 0, BiCGSTAB's first stop test, rho' = -0 * 0
    B  a zero denominator under a non-zero numerator (an operator that is identically zero): x/0 -> inf -> 0
    C  one unknown (3 nodes per axis): every sum has one term
    D  a right-hand side with ONE non-zero cell, moved over the places where a kernel changes hands: r.r, d.Ad and
       |dx|^2 are one-term (next to a neumann / symmetry face: two-term) sums

A case is a dict: name, family, mesh (a key of MESHES), n, dtype, bcs [(type, value)] in face order, method, tol, max_it,
eq ("lap", 0.8 | 0.0 | "zeros") or ("div", 0.6), rhs / x0 (recipes of ``inputs``), free -- what of the run has no summation
order: "all" (every summed product has at most two non-zero terms), "zero_den" (x, itr, tol and the raise do not depend
on the sums because the denominator is exactly zero), "start" (BiCGSTAB, family D: r0.r0 and r0.v only) -- and keys: the
entries of ``ctx.scalars()`` that are demanded bit for bit.
"""
import contextlib
import warnings

import numpy as np
import torch

import pyapes_oracle as O
from edge_fields import distinct_positions, planted
from helpers import SumTap, sum_order

TDT = {"single": torch.float32, "double": torch.float64}
NPT = {"single": np.float32, "double": np.float64}
BOTH = ("double", "single")
METHODS = ("cg", "jacobi", "bicgstab")

# ---- meshes ---------------------------------------------------------------------------------------------------------------
# name: (nodes, dtypes, kind).  The kind names the paths a mesh admits (PATHS); which kernel really ran is read from the
# launch log and from resident_used / resident_plan by the GPU test.
MESHES = {
    "g3": ([6, 7, 9], BOTH, "small"),
    "g2": ([17, 12], BOTH, "small"),
    "r3": ([20, 18, 22], BOTH, "small"),      # resident: a plan of more than one box
    "r2": ([40, 36], BOTH, "small"),
    "t64": ([10, 12, 132], ("double",), "tiled"),
    "t32": ([12, 18, 132], ("single",), "tiled"),
    "m2": ([12, 40], BOTH, "cg2d"),           # k_cg2d with cg2d_mincells lowered (tests/test_gpu_cg2d.py, test_gpu_fold.py)
    "p3": ([6, 9, 13], BOTH, "oddrow"),       # odd rows: the pitched layout (tests/test_gpu_pitched.py, test_gpu_fold.py)
    "c1": ([3], BOTH, "small"),
    "c2": ([3, 3], BOTH, "small"),
    "c3": ([3, 3, 3], BOTH, "small"),
}
RESIDENT_MESHES = ("r3", "r2")     # the plan must take these with more than one box (a periodic axis is never cut: one box)

# ---- paths ----------------------------------------------------------------------------------------------------------------
# name: options of the context (pa_ctx_set_option); "stepwise": cg_begin + cg_iterate(K) + cg_end instead of Solver.solve
_LPP = {"resident": 0}
PATHS = {
    "small": {
        "generic": dict(_LPP, fastpath=0, fold=0),
        "fast_fold1": dict(_LPP, fastpath=1, fold=1),
        "fast_fold0": dict(_LPP, fastpath=1, fold=0),
        "resident": {"resident": 1},
    },
    "tiled": {
        "generic": dict(_LPP, fastpath=0, fold=0),
        "chunks1_fold1": dict(_LPP, fastpath=1, fold=1, chunks=1),
        "chunks2_fold1": dict(_LPP, fastpath=1, fold=1, chunks=2),
        "chunks2_fold0": dict(_LPP, fastpath=1, fold=0, chunks=2),
    },
    "cg2d": {
        "generic": dict(_LPP, fastpath=0, fold=0),
        "cg2d_fold1": dict(_LPP, fastpath=1, fold=1, cg2d_mincells=0),
        "cg2d_fold0": dict(_LPP, fastpath=1, fold=0, cg2d_mincells=0),
        "plane_fold1": dict(_LPP, fastpath=1, fold=1, cg2d_mincells=-1),
    },
    "oddrow": {
        "generic": dict(_LPP, fastpath=0, fold=0),
        "pitch1_fold1": dict(_LPP, fastpath=1, fold=1, pitch=1),
        "pitch1_fold0": dict(_LPP, fastpath=1, fold=0, pitch=1),
        "pitch0_fold1": dict(_LPP, fastpath=1, fold=1, pitch=0),
    },
}
# the stepwise entry points exist for CG: the path a CG case runs besides those of its mesh
STEPWISE = {"small": "fast_fold1", "tiled": "chunks2_fold1", "cg2d": "cg2d_fold1", "oddrow": "pitch1_fold1"}
STEPWISE_EXTRA = 3     # cg_iterate(K): K = this many iterations more than the solve can run


def paths_of(case):
    """[(path name, options, stepwise)] of a case"""
    kind = MESHES[case["mesh"]][2]
    out = [(name, opts, False) for name, opts in PATHS[kind].items()]
    if case["method"] == "cg":
        out.append(("stepwise", PATHS[kind][STEPWISE[kind]], True))
    return out


# (case, path) pairs that do not apply: [(predicate on the case, path name, reason)].  The GPU test asserts for each of
# them that the path really is not taken (resident_plan == 0), so an entry that has become wrong is noticed.
NOT_APPLICABLE = [
    (lambda c: c["mesh"] == "r3" and c["bcs"][0][0] == "periodic", "resident",
     "a periodic axis is never cut, and 20 x 18 x 22 uncut does not fit one workgroup's LDS: the launch-per-phase loops run"),
    (lambda c: c["mesh"] in ("c1", "c2", "c3"), "resident",
     "the resident plan needs at least 5 nodes on every axis (res_applicable): a 3-node mesh runs the launch-per-phase loops"),
]


def not_applicable(case, path):
    """the reason string of a (case, path) pair that does not apply, else None"""
    for pred, name, reason in NOT_APPLICABLE:
        if name == path and pred(case):
            return reason
    return None


# ---- face sets ------------------------------------------------------------------------------------------------------------
def _dir(v, nd):
    return [("dirichlet", v)] * (2 * nd)


# zero values; xu / zl neumann, yl symmetry: the centre lines of a mesh pass next to a neumann and a symmetry face
MIXED0 = [("dirichlet", 0.0), ("neumann", 0.0), ("symmetry", None), ("dirichlet", 0.0), ("neumann", 0.0), ("dirichlet", 0.0)]
PERIODIC = [("periodic", None)] * 6
DISTINCT = [("dirichlet", v) for v in (0.25, -0.5, 0.75, 0.125, -0.375, 1.5)]


def face_set(name, nd):
    return {"dir0": _dir(0.0, nd), "dir03": _dir(0.3, nd), "dir01": _dir(0.1, nd), "mixed0": MIXED0[:2 * nd],
            "periodic": PERIODIC[:2 * nd], "distinct": DISTINCT[:2 * nd]}[name]


# ---- the table ------------------------------------------------------------------------------------------------------------
CG_KEYS = ("alpha", "beta", "rr", "dAd")
BICG_KEYS = ("alpha", "beta", "rho", "omega", "rho_next")
ALL_KEYS = {"cg": CG_KEYS, "jacobi": (), "bicgstab": BICG_KEYS}


def _case(family, mesh, dtype, bcname, method, tol, max_it, eq, rhs, x0, free, keys, tag):
    n = MESHES[mesh][0]
    return dict(name="%s-%s%s-%s-%s-%s" % (family, mesh, dtype[0], bcname, method, tag), family=family, mesh=mesh, n=list(n),
                dtype=dtype, bcname=bcname, bcs=face_set(bcname, len(n)), method=method, tol=tol, max_it=max_it, eq=eq, rhs=rhs,
                x0=x0, free=free, keys=tuple(keys))


A_MESHES = ("g3", "g2", "r3", "r2", "t64", "t32", "m2", "p3")
A_INPUTS = (("dir0", 0.0), ("mixed0", 0.0), ("periodic", 0.0), ("dir03", 0.3))
A_TOLS = (1e-6, 0.0, -1.0)


def family_a():
    out = []
    for mesh in A_MESHES:
        for dtype in MESHES[mesh][1]:
            for bcname, fill in A_INPUTS:
                for tol in A_TOLS:
                    for method in METHODS:
                        out.append(_case("A", mesh, dtype, bcname, method, tol, 5, ("lap", 0.8), ("zero",), ("const", fill),
                                         "all", ALL_KEYS[method], "tol%g" % tol))
    return out


B_MESHES = ("g3", "g2", "r3", "t64", "t32")


def family_b():
    """random rhs / x0, Dirichlet 0.1 faces, an operator that is zero; and (CG, BiCGSTAB) a lone central Div, whose
    diagonal is zero, under a one-cell right-hand side"""
    out = []
    for mesh in B_MESHES:
        for dtype in MESHES[mesh][1]:
            for eq in (("lap", 0.0), ("lap", "zeros")):
                for tol in (1e-6, -1.0):
                    for method in METHODS:
                        # CG: alpha = (r.r) / 0 -> 0 whatever r.r is; beta = r'.r' / r.r has a summation order (r' = r, but the
                        # two sums are formed by different kernels) and feeds nothing that is compared
                        keys = ("alpha",) if method == "cg" else ()
                        out.append(_case("B", mesh, dtype, "dir01", method, tol, 5, eq, ("randn", 31), ("randn", 32),
                                         "zero_den", keys, "%s-tol%g" % (eq[1], tol)))
    for mesh in ("g3", "g2"):
        for dtype in MESHES[mesh][1]:
            for method in ("cg", "bicgstab"):
                n = MESHES[mesh][0]
                out.append(_case("B", mesh, dtype, "dir0", method, 1e-6, 5, ("div", 0.6), ("cell", tuple(m // 2 for m in n)),
                                 ("const", 0.0), "all" if method == "cg" else "zero_den",
                                 ("alpha", "dAd") if method == "cg" else ("alpha", "rr"), "div"))
    return out


def family_c():
    out = []
    for mesh in ("c1", "c2", "c3"):
        for dtype in MESHES[mesh][1]:
            for max_it in range(5):
                for method in METHODS:
                    out.append(_case("C", mesh, dtype, "distinct", method, -1.0, max_it, ("lap", 0.8), ("randn", 41),
                                     ("randn", 42), "all", ALL_KEYS[method], "k%d" % max_it))
    return out


def axis_lines(n):
    """every index along the axis lines through the mesh centre: crosses every cut of a box plan, wherever it is"""
    mid = [m // 2 for m in n]
    seen = []
    for a in range(len(n)):
        for i in range(n[a]):
            p = tuple(i if q == a else mid[q] for q in range(len(n)))
            if p not in seen:
                seen.append(p)
    return seen


def d_positions(mesh, dtype):
    n = MESHES[mesh][0]
    if MESHES[mesh][2] == "tiled":
        seen = []
        for chunks in (1, 2):
            for _, at in distinct_positions(n, dtype, chunks):
                if at not in seen:
                    seen.append(at)
        return seen
    return axis_lines(n)


D_MESHES = (("t64", ("dir0", "mixed0")), ("t32", ("dir0", "mixed0")), ("r3", ("mixed0",)))


def family_d():
    """CG / Jacobi: max_it = 0, one iteration; BiCGSTAB: max_it = 1, where only r0.r0 (`rr`), r0.v and alpha = rr / r0.v
    have no summation order (the library overwrites `rho` with rho' = -omega (r0.t) when it closes the iteration, and only
    some of its paths keep r0.v itself in the state: alpha carries it)"""
    out = []
    for mesh, sets in D_MESHES:
        for dtype in MESHES[mesh][1]:
            for bcname in sets:
                for at in d_positions(mesh, dtype):
                    tag = "at" + "_".join(map(str, at))
                    out.append(_case("D", mesh, dtype, bcname, "cg", -1.0, 0, ("lap", 0.8), ("cell", at), ("const", 0.0), "all",
                                     ("alpha", "dAd", "rr_old"), tag))
                    out.append(_case("D", mesh, dtype, bcname, "jacobi", -1.0, 0, ("lap", 0.8), ("cell", at), ("const", 0.0),
                                     "all", (), tag))
                    out.append(_case("D", mesh, dtype, bcname, "bicgstab", -1.0, 1, ("lap", 0.8), ("cell", at), ("const", 0.0),
                                     "start", ("alpha", "rr"), tag))
    return out


def audit_case(mesh, dtype):
    """the solve whose launch log shows which kernels a (mesh, dtype, path) runs: two CG iterations, random fields"""
    return _case("audit", mesh, dtype, "dir01", "cg", -1.0, 1, ("lap", 0.8), ("randn", 61), ("randn", 62), "none", (), "log")


_TABLE = {}


def cases(family=None):
    if not _TABLE:
        for fam, build in (("A", family_a), ("B", family_b), ("C", family_c), ("D", family_d)):
            _TABLE[fam] = build()
        names = [c["name"] for f in _TABLE.values() for c in f]
        assert len(names) == len(set(names))
    return [c for f in _TABLE.values() for c in f] if family is None else _TABLE[family]


# ---- the outcomes the oracle gives, pinned: a change of the oracle is noticed ---------------------------------------------
# (family, method, tol class) -> (itr, tol, converge) or "raises"; K = max_it.  Family C has no row: the oracle decides each
# of its outcomes (test_degenerate_host pins the one quoted figure: CG on 3^3 raises from max_it = 2).
def pinned_outcome(case):
    fam, method, tol, K = case["family"], case["method"], case["tol"], case["max_it"]
    if fam == "A":
        if tol >= 0:
            return (1, 0.0, True)                 # x unchanged
        return (K + 1, 0.0, False) if method == "jacobi" else "raises"     # d = r + NaN d, then x + 0 NaN
    if fam == "B" and case["eq"][0] == "lap":
        if method == "cg":
            return (1, 0.0, True) if tol >= 0 else (K + 1, 0.0, False)     # the BC-filled x0
        return "raises"                           # Jacobi: tol = inf; BiCGSTAB: NaN
    if fam == "B":
        return (1, 0.0, True) if method == "cg" else "raises"
    if fam == "D":
        return (1, None, False)                   # one iteration; tol is the case's own
    return None


# ---- builders -------------------------------------------------------------------------------------------------------------
def lengths(nd):
    return [1.0 + 0.1 * a for a in range(nd)]


def oracle_mesh(case):
    nd = len(case["n"])
    return O.OMesh([0.0] * nd, lengths(nd), list(case["n"]), case["dtype"], "xyz")


def oracle_cfg(case):
    return [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(case["bcs"])]


def _field(spec, n, dtype):
    tdt, shape = TDT[dtype], (1, *n)
    if spec[0] == "zero":
        return torch.zeros(shape, dtype=tdt)
    if spec[0] == "const":
        return torch.full(shape, spec[1], dtype=tdt)
    if spec[0] == "randn":
        g = torch.Generator().manual_seed(spec[1])
        return torch.randn(shape, generator=g, dtype=torch.float64).to(tdt)
    if spec[0] == "cell":
        return planted(torch.zeros(shape, dtype=tdt), 1.75, spec[1])
    raise ValueError(spec)


def inputs(case):
    """(rhs, x0) on the CPU, fresh tensors"""
    return _field(case["rhs"], case["n"], case["dtype"]), _field(case["x0"], case["n"], case["dtype"])


def coefficient(case):
    """the Laplacian's coefficient: a number, or the all-zero tensor"""
    c = case["eq"][1]
    return torch.zeros((1, *case["n"]), dtype=TDT[case["dtype"]]) if c == "zeros" else c


class TermTap:
    """Records, for every ``torch.sum(t, dim=...)`` made while it is active, (finite non-zero terms, non-finite terms) of
    ``t``.  A sum with a non-finite term has no order either: it is NaN or an infinity whatever the grouping, unless finite
    terms alone would overflow, which the O(1) fields of these cases do not."""

    def __init__(self):
        self.terms = []

    def __enter__(self):
        self.prev = torch.sum
        prev, terms = self.prev, self.terms

        def tap(t, dim=None, **kw):
            if dim is not None:
                fin = torch.isfinite(t)
                terms.append((int((fin & (t != 0)).sum()), int((~fin).sum())))
            return prev(t, dim=dim, **kw) if dim is not None else prev(t, **kw)

        torch.sum = tap
        return self

    def __exit__(self, *exc):
        torch.sum = self.prev


def oracle_run(case, variant=0, taps=()):
    """The oracle on a case -> dict(x, itr, tol, converge, raised): ``raised`` is the message of the RuntimeError, x / itr /
    tol / converge are None then.  ``variant``: helpers.sum_order; ``taps``: context managers that go on after it, in order
    (and come off before it: each restores the ``torch.sum`` it found)."""
    rhs, x0 = inputs(case)
    mesh, cfg = oracle_mesh(case), oracle_cfg(case)
    with sum_order(variant), warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        with contextlib.ExitStack() as stack:
            for t in taps:
                stack.enter_context(t)
            try:
                if case["eq"][0] == "lap":
                    x, rep = O.solve_poisson(mesh, cfg, rhs, x0=x0, method=case["method"], tol=case["tol"],
                                             max_it=case["max_it"], coeff=coefficient(case), sign=-1.0)
                else:
                    spec = [{"kind": "div", "sign": 1.0, "u": case["eq"][1], "limiter": "none"}]
                    x, rep = O.solve_equation(mesh, cfg, spec, rhs, x0=x0, method=case["method"], tol=case["tol"],
                                              max_it=case["max_it"])
            except RuntimeError as e:
                return dict(x=None, itr=None, tol=None, converge=None, raised=str(e))
    return dict(x=x, itr=int(rep["itr"]), tol=float(rep["tol"]), converge=bool(rep["converge"]), raised=None)


_ORACLE = {}


def oracle(case):
    """``oracle_run`` of the case in torch's own summation order with its tapped sums (``sums``), their term counts
    (``terms``, see TermTap) and the scalars the library must hold at the end (``scalars``): computed once, shared, not to
    be changed"""
    if case["name"] not in _ORACLE:
        terms, tap = TermTap(), SumTap()
        out = oracle_run(case, 0, (terms, tap))          # (SumTap goes on last: it records what the sums return)
        out["sums"], out["terms"] = list(tap.vals), list(terms.terms)
        out["scalars"] = expected_scalars(case["method"], out["sums"], case["dtype"], out["raised"] is not None)
        _ORACLE[case["name"]] = out
    return _ORACLE[case["name"]]


def first_residual(case):
    """rhs (adjusted) - A x0 on the interior set, x0 BC-filled: what the loops start from"""
    rhs, x = inputs(case)
    mesh = oracle_mesh(case)
    bcs = O.make_bcs(mesh, oracle_cfg(case))
    tabs = O.laplacian_tables(x, mesh, bcs)
    rhs += O.laplacian_rhs_adjust(x, mesh, bcs)
    O.bc_fill(x, bcs)
    S = O.interior_slicer(mesh.dim, bcs)
    r = torch.zeros_like(x)
    r[0][S] = rhs[0][S] - O.Aop(x, [O.OTerm("laplacian", tabs, coefficient(case), -1.0)], mesh.dim)[0][S]
    return r


def expected_scalars(method, sums, dtype, raised):
    """The entries of ``ctx.scalars()`` after the run whose dot products are ``sums`` (a SumTap of the oracle), as far as the
    run determines them.  The cast: every tapped sum is a number of the mesh's precision already (the oracle sums tensors
    of that dtype), and every quotient and product is formed in that precision (numpy scalars), as the oracle forms them
    on tensors and pa_scalar_steps.h on ``T`` -- helpers.scalar_history forms them in Python doubles, which for a quotient
    of two fp32 numbers rounds to the same fp32 number (53 >= 2 * 24 + 2 bits), but not for rho' = -omega (r0.t).

    CG (linalg.py:118-141): per iteration r.r, d.Ad, r.r, r'.r'; a raise comes after the third.  BiCGSTAB
    (linalg.py:204-250): r0.r0, then per iteration r0.v and -- unless the first stop test ends or raises -- t.s, t.t, r0.t.
    The library forms the next beta, and moves rho' into rho, when it CLOSES an iteration (pa_step_bicg_close), the
    reference at the top of the next one: after a run that ends on a closed iteration that step is applied once more."""
    f = NPT[dtype]

    def nn(v):
        return f(0.0) if not np.isfinite(v) else v

    out = {}
    with np.errstate(all="ignore"):
        if method == "cg":
            i = 0
            if sums:
                out["rr"] = f(sums[0])
            while i + 1 < len(sums):
                out["dAd"] = f(sums[i + 1])
                out["alpha"] = nn(f(sums[i]) / out["dAd"])
                if i + 3 < len(sums):
                    out["rr_old"] = f(sums[i + 2])
                    out["rr"] = f(sums[i + 3])
                    out["beta"] = out["rr"] / out["rr_old"]
                i += 4
        elif method == "bicgstab":
            rho, alpha, omega, rho_next = f(1.0), f(1.0), f(1.0), f(sums[0])
            out["rr"] = f(sums[0])
            i, closed = 1, False
            beta = None
            while i < len(sums):
                beta = rho_next / rho * alpha / omega
                rho = rho_next
                out["r0v"] = f(sums[i])
                alpha = nn(rho / out["r0v"])
                closed = False
                if len(sums) - i >= 4:
                    omega = nn(f(sums[i + 1]) / f(sums[i + 2]))
                    rho_next = -omega * f(sums[i + 3])
                    closed = True
                    i += 4
                else:
                    i += 1
            if closed and not raised:
                beta = rho_next / rho * alpha / omega
                rho = rho_next
            out.update(alpha=alpha, omega=omega, rho=rho, rho_next=rho_next)
            if beta is not None:
                out["beta"] = beta
    return {k: float(v) for k, v in out.items()}


# ---- context reuse: an ordinary solve after a degenerate ending -----------------------------------------------------------
# ending: (family, a selector of one case per mesh / dtype).  The follow-up: random rhs / x0 on the same face set,
# tol = -1, six iterations, every method.
REUSE_ENDINGS = {
    "zero_start_returned": lambda c: c["family"] == "A" and c["tol"] == 1e-6 and c["bcname"] == "mixed0",
    "zero_start_raised": lambda c: c["family"] == "A" and c["tol"] == -1.0 and c["bcname"] == "dir03" and c["method"] != "jacobi",
    "zero_operator_cg": lambda c: c["family"] == "B" and c["eq"] == ("lap", 0.0) and c["tol"] == -1.0 and c["method"] == "cg",
    "one_unknown_raised": lambda c: c["family"] == "C" and c["max_it"] == 4 and c["method"] != "jacobi",
}
REUSE_MESHES = {"zero_start_returned": ("g3", "r3", "t64", "m2"), "zero_start_raised": ("g2", "r3", "t32", "p3"),
                "zero_operator_cg": ("g3", "r3", "t64"), "one_unknown_raised": ("c2", "c3")}


def reuse_cases(ending):
    sel = REUSE_ENDINGS[ending]
    if ending == "one_unknown_raised":   # the oracle decides which of them raise: both precisions, those that do
        return [c for c in cases("C") if sel(c) and c["mesh"] in REUSE_MESHES[ending] and oracle(c)["raised"] is not None]
    return [c for c in cases() if sel(c) and c["mesh"] in REUSE_MESHES[ending]
            and c["dtype"] == MESHES[c["mesh"]][1][0]]


def follow_up(case, method):
    """the ordinary solve that follows ``case`` on its mesh: same face set, -0.8 laplacian, random fields"""
    return dict(case, name=case["name"] + "+" + method, method=method, tol=-1.0, max_it=6 if method == "bicgstab" else 5,
                eq=("lap", 0.8), rhs=("randn", 51), x0=("randn", 52), keys=(), free="none", family="reuse")
