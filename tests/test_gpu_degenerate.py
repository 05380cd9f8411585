"""-m gpu: the solver loops where their scalars degenerate (tests/degenerate_cases.py: zero residual at the start, a zero
denominator, one unknown, a one-cell right-hand side), on every solver path -- generic and tiled kernels, chunk counts,
the 2-D marching kernel, pitched rows, folded and unfolded scalar steps, the resident loop, the stepwise entry points --
against the CPU oracle BIT FOR BIT: tests/test_degenerate_host.py proves that the oracle's own result has no summation
order on these inputs, so no grouping of the partial sums excuses a difference.

Per (case, path): x, itr, converge and the raise are the oracle's; tol is 0.0 where the oracle's is, else within the
bounds of tests/test_gpu_resident.py (the oracle's goes through torch.linalg.norm, which need not be sqrt(sum of
squares) in the last bit); the scalars named by the case are the ones restated from the oracle's tapped sums in the
mesh's precision (degenerate_cases.expected_scalars says which cast and why).  Per case: tol and those scalars are the
same bits on all paths."""
import os
import re
import subprocess
import sys
import warnings

import pytest
import torch

import degenerate_cases as DC
from helpers import same_bits

pytestmark = pytest.mark.gpu

XTOL = {"double": 1e-11, "single": 2e-4}        # x where a sum has an order (family D, BiCGSTAB): the suite's bounds
TOL_REL = {"double": 1e-9, "single": 1e-3}      # tol against the oracle's (tests/test_gpu_resident.py)
SCALAR_NAMES = ("alpha", "beta", "rr", "rr_old", "dAd", "tol", "rho", "omega", "rho_next", "r0v", "ts", "tt", "r0t", "itr")


def _same_float(a, b):
    return bool(same_bits(torch.tensor([a], dtype=torch.float64), torch.tensor([b], dtype=torch.float64)))


def gpu_run(case, opts, stepwise=False, mesh=None):
    """The case through the library with the context options ``opts`` -> dict(x, itr, tol, converge, raised, scalars, used,
    plan, mesh).  ``stepwise``: cg_begin + cg_iterate(K) + cg_end with K beyond the iteration that ends the solve -- what
    is enqueued after `done` must change nothing.  ``mesh``: solve on this mesh (and its context) instead of a fresh one."""
    from pyapes_amd.geometry import Box
    from pyapes_amd.hip.context import context_for
    from pyapes_amd.mesh import Mesh
    from pyapes_amd.solver.fdm import FDM
    from pyapes_amd.solver.linalg import terms_of
    from pyapes_amd.solver.ops import Solver
    from pyapes_amd.variables import Field
    import pyapes_oracle as O
    nd = len(case["n"])
    if mesh is None:
        mesh = Mesh(Box([0.0] * nd, DC.lengths(nd)), None, list(case["n"]), "cuda", case["dtype"])
    ctx = context_for(mesh)
    for k, v in opts.items():
        ctx.set_option(k, v)
    cfg = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v, "bc_val_opt": None} for i, (t, v) in enumerate(case["bcs"])]
    var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
    rhs, x0 = DC.inputs(case)
    var.set_var_tensor(x0.cuda())
    s = Solver({"fdm": {"method": case["method"], "tol": case["tol"], "max_it": case["max_it"], "report": False}})
    if case["eq"][0] == "lap":
        coeff = DC.coefficient(case)
        eq = -FDM().laplacian(coeff.cuda() if isinstance(coeff, torch.Tensor) else coeff, var)
    else:
        eq = FDM({"div": {"limiter": "none", "edge": False}}).div(case["eq"][1], var)
    s.set_eq(eq == rhs.cuda())
    out = dict(x=None, itr=None, tol=None, converge=None, raised=None, mesh=mesh)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            if stepwise:
                assert case["method"] == "cg"
                terms, _ = terms_of(s.eqs)
                ctx.bind_bcs(var(), var.bcs, 0)
                ctx.set_terms(terms)
                out["plan"] = (0, (0, 0, 0))
                ctx.cg_begin(var()[0], s.rhs[0], case["tol"], case["max_it"])
                try:
                    ctx.cg_iterate(case["max_it"] + 1 + DC.STEPWISE_EXTRA)
                except BaseException:
                    ctx.cg_abort()
                    raise
                rep = ctx.cg_end()
                rep = {"itr": int(rep.itr), "tol": float(rep.tol), "converge": bool(rep.itr < case["max_it"])}
                out["used"] = 0
            else:
                rep = s.solve()
                out["used"] = ctx.resident_used()
            out.update(x=var().cpu(), itr=int(rep["itr"]), tol=float(rep["tol"]), converge=bool(rep["converge"]))
        except RuntimeError as e:
            out["raised"] = str(e)
            out["used"] = 0 if stepwise else ctx.resident_used()
    if not stepwise:
        out["plan"] = ctx.resident_plan(case["method"])
    out["scalars"] = ctx.scalars()
    return out


def check_against_oracle(case, pname, r):
    o = DC.oracle(case)
    who = (case["name"], pname)
    if o["raised"] is not None:
        assert r["raised"] is not None and "Invalid tolerance" in r["raised"], (who, r["raised"], r["itr"], r["tol"])
    else:
        assert r["raised"] is None, (who, r["raised"])
        assert (r["itr"], r["converge"]) == (o["itr"], o["converge"]), (who, r["itr"], r["converge"], o["itr"], o["converge"])
        if case["free"] == "start":
            err, scale = float((r["x"] - o["x"]).abs().max()), float(o["x"].abs().max())
            assert err <= XTOL[case["dtype"]] * scale, (who, err, scale)
        else:
            assert same_bits(r["x"], o["x"]), (who, same_bits(r["x"], o["x"]))
        if o["tol"] == 0.0:
            assert r["tol"] == 0.0, (who, r["tol"])
        else:
            assert abs(r["tol"] - o["tol"]) <= TOL_REL[case["dtype"]] * abs(o["tol"]), (who, r["tol"], o["tol"])
    for key in case["keys"]:
        if key in o["scalars"]:
            assert _same_float(r["scalars"][key], o["scalars"][key]), (who, key, r["scalars"][key], o["scalars"][key])


def check_path_taken(case, pname, r):
    """resident_used / resident_plan say whether the resident loop ran; tests below read the launch log for the kernels"""
    who = (case["name"], pname)
    if pname != "resident":
        assert r["used"] == 0, (who, r["used"])
        return
    if DC.not_applicable(case, pname) is not None:
        assert r["used"] == 0 and r["plan"][0] == 0, (who, r["used"], r["plan"])
        return
    assert r["used"] > 0 and r["used"] == r["plan"][0], (who, r["used"], r["plan"])
    if case["mesh"] in DC.RESIDENT_MESHES and case["bcname"] != "periodic":
        assert r["plan"][0] > 1, (who, r["plan"])


def check_case(case):
    runs = {}
    for pname, opts, stepwise in DC.paths_of(case):
        r = gpu_run(case, opts, stepwise)
        check_path_taken(case, pname, r)
        check_against_oracle(case, pname, r)
        runs[pname] = r
    first_name = next(iter(runs))
    first = runs[first_name]
    for pname, r in runs.items():
        who = (case["name"], first_name, pname)
        assert (r["raised"] is None) == (first["raised"] is None), who
        if case["free"] != "start" and first["raised"] is None:   # (family D's BiCGSTAB: |s| and |r| have an order)
            assert _same_float(r["tol"], first["tol"]), (who, r["tol"], first["tol"])
        for key in case["keys"]:
            assert _same_float(r["scalars"][key], first["scalars"][key]), (who, key, r["scalars"][key], first["scalars"][key])
    return runs


# eight cases per test: a test here is to stay below the slowest test of tests/test_gpu_resident.py (~0.2 s)
PER_TEST = 8


def _chunks():
    groups = {}
    for c in DC.cases():
        groups.setdefault((c["family"], c["mesh"], c["dtype"]), []).append(c["name"])
    return [("%s-%s-%s-%d" % (*g, i // PER_TEST), names[i:i + PER_TEST])
            for g, names in sorted(groups.items()) for i in range(0, len(names), PER_TEST)]


CHUNKS = _chunks()
BY_NAME = {c["name"]: c for c in DC.cases()}


@pytest.mark.parametrize("names", [n for _, n in CHUNKS], ids=[i for i, _ in CHUNKS])
def test_degenerate_cases_on_every_path(names):
    for name in names:
        check_case(BY_NAME[name])


def test_every_case_is_in_one_chunk():
    seen = [n for _, names in CHUNKS for n in names]
    assert sorted(seen) == sorted(BY_NAME) and len(seen) == len(set(seen))


def test_every_path_has_a_case_in_every_family():
    """what the table sends where (the per-pair assertions above and the launch logs below show that it arrives): every
    family runs the generic kernels, the tiled ones folded and unfolded, the resident loop and the stepwise entry points;
    the families with a tiled mesh both chunk counts; family A the marching kernel and both layouts of odd rows too"""
    for fam in "ABCD":
        seen = {(DC.MESHES[c["mesh"]][2], p) for c in DC.cases(fam) for p, _, _ in DC.paths_of(c)
                if DC.not_applicable(c, p) is None}
        names = {p for _, p in seen}
        assert {"generic", "stepwise"} <= names, (fam, names)
        assert "resident" in names or fam == "C", (fam, names)      # (one unknown: NOT_APPLICABLE says why)
        assert any(p.endswith("fold1") for p in names) and any(p.endswith("fold0") for p in names), (fam, names)
        if fam != "C":
            assert {"chunks1_fold1", "chunks2_fold1", "chunks2_fold0"} <= names, (fam, names)
        if fam == "A":
            assert {"cg2d_fold1", "cg2d_fold0", "plane_fold1", "pitch1_fold1", "pitch1_fold0", "pitch0_fold1"} <= names, names


# ---- which kernels ran: the launch log --------------------------------------------------------------------------------------
# (mesh kind, path) -> what the log of a CG solve must show for its phases A and B: None -- no tiled phase at all (the
# generic kernels) --, (kernel, layout tag or None for any, chunk count or None for any), or "any": the launcher decides
# by the mesh (3-D meshes down to 3 nodes per axis run k_cg3d, small 2-D meshes the generic phases), one kernel for both.
LOG = {
    ("tiled", "generic"): None, ("tiled", "chunks1_fold1"): ("k_cg3d", None, 1), ("tiled", "chunks2_fold1"): ("k_cg3d", None, 2),
    ("tiled", "chunks2_fold0"): ("k_cg3d", None, 2),
    ("cg2d", "generic"): None, ("cg2d", "cg2d_fold1"): ("k_cg2d", None, None), ("cg2d", "cg2d_fold0"): ("k_cg2d", None, None),
    ("cg2d", "plane_fold1"): "any",
    ("oddrow", "generic"): None, ("oddrow", "pitch1_fold1"): ("k_cg3d", "pitched", None),
    ("oddrow", "pitch1_fold0"): ("k_cg3d", "pitched", None), ("oddrow", "pitch0_fold1"): ("k_cg3d", "narrow", None),
    ("small", "generic"): None, ("small", "fast_fold1"): "any", ("small", "fast_fold0"): "any",
}
_LINE = re.compile(r"(k_cg3d|k_cg2d) phase ([A-Z])(?: \((\w+)\))?:(?: tiles \S+ chunks (\d+))?")


def audit_solves(kind):
    """[(marker, mesh, dtype, path, options)] of one mesh kind"""
    out = []
    for mesh, (n, dtypes, k) in DC.MESHES.items():
        if k != kind:
            continue
        for dtype in dtypes:
            for pname, opts in DC.PATHS[kind].items():
                if pname != "resident":
                    out.append(("%s %s %s" % (mesh, dtype, pname), mesh, dtype, pname, opts))
    return out


def _audit_child(kind):
    def mark(s):
        sys.stderr.write("CASE " + s + "\n")
        sys.stderr.flush()

    for marker, mesh, dtype, pname, opts in audit_solves(kind):
        mark(marker)
        r = gpu_run(DC.audit_case(mesh, dtype), opts)
        assert r["raised"] is None and r["itr"] == 2, (marker, r["raised"], r["itr"])
    mark("end")


@pytest.mark.parametrize("kind", sorted(DC.PATHS))
def test_launch_log_names_the_kernels(kind):
    """one child process per mesh kind (the log is limited per kernel instantiation and process), a marker per solve"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys\nfor p in (%r, %r, %r): sys.path.insert(0, p)\n"
            "import test_gpu_degenerate as T\nT._audit_child(%r)\n"
            % (root, os.path.join(root, "oracle"), os.path.join(root, "tests"), kind))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, PYAPES_HIP_DEBUG="1"))
    assert p.returncode == 0, p.stderr[-3000:]
    logs = {seg.split("\n", 1)[0].strip(): seg for seg in p.stderr.split("CASE ")[1:]}
    solves = audit_solves(kind)
    assert set(logs) == {s[0] for s in solves} | {"end"}
    tiled_ab = {}
    for marker, mesh, dtype, pname, opts in solves:
        every = _LINE.findall(logs[marker])
        lines = [l for l in every if l[1] in "AB"]      # (phase C, the first residual, is laid out by its own rule)
        want = LOG[(kind, pname)]
        if want is None:
            assert not every, (marker, every)
            continue
        if want == "any":
            assert not lines or ({ph for k, ph, t, ch in lines} == {"A", "B"} and len({k for k, ph, t, ch in lines}) == 1), (marker, lines)
            tiled_ab[kind] = tiled_ab.get(kind, 0) + (1 if lines else 0)
            continue
        kernel, tag, chunks = want
        assert {ph for k, ph, t, ch in lines} == {"A", "B"}, (marker, every, logs[marker][-1500:])
        assert all(k == kernel for k, ph, t, ch in lines), (marker, lines)
        if tag is not None:
            assert all(t == tag for k, ph, t, ch in lines), (marker, lines)
        if chunks is not None:
            assert all(ch == str(chunks) for k, ph, t, ch in lines), (marker, lines)
    if kind == "small":   # the 3-D meshes of the kind: fastpath 1 is no other name for the generic kernels
        assert tiled_ab.get(kind, 0) >= 2, tiled_ab


# ---- the context after a degenerate ending ----------------------------------------------------------------------------------
REUSE = [(e, c["name"]) for e in sorted(DC.REUSE_ENDINGS) for c in DC.reuse_cases(e)]


@pytest.mark.parametrize("ending,name", REUSE, ids=["%s-%s" % r for r in REUSE])
def test_an_ordinary_solve_follows_a_degenerate_ending(ending, name):
    """after each kind of degenerate ending, on every path: one ordinary solve per method on the SAME mesh and context
    equals the same solve on a fresh mesh in every bit -- x, itr, tol, all the scalars, or the raise (same path, same
    grouping of the sums: nothing excuses a difference; a NaN beta or direction buffer left behind would show here)"""
    for case in [BY_NAME[name]]:
        o = DC.oracle(case)
        for pname, opts, stepwise in DC.paths_of(case):
            first = gpu_run(case, opts, stepwise)
            assert (first["raised"] is not None) == (o["raised"] is not None), (ending, case["name"], pname, first["raised"])
            mesh = first["mesh"]
            for method in DC.METHODS:
                f = DC.follow_up(case, method)
                step = stepwise and method == "cg"
                used = gpu_run(f, opts, step, mesh=mesh)
                fresh = gpu_run(f, opts, step)
                who = (ending, case["name"], pname, method)
                assert used["raised"] == fresh["raised"] or (used["raised"] and fresh["raised"]
                                                             and "Invalid tolerance" in used["raised"]
                                                             and "Invalid tolerance" in fresh["raised"]), (who, used["raised"], fresh["raised"])
                assert used["used"] == fresh["used"], (who, used["used"], fresh["used"])
                if fresh["raised"] is None:
                    assert same_bits(used["x"], fresh["x"]), (who, same_bits(used["x"], fresh["x"]))
                    assert used["itr"] == fresh["itr"] and _same_float(used["tol"], fresh["tol"]), (who, used["itr"], fresh["itr"], used["tol"], fresh["tol"])
                    if case["family"] != "C":
                        assert fresh["itr"] == 6 and fresh["tol"] > 0, (who, fresh["itr"], fresh["tol"])
                for key in SCALAR_NAMES:
                    assert _same_float(used["scalars"][key], fresh["scalars"][key]), (who, key, used["scalars"][key], fresh["scalars"][key])
