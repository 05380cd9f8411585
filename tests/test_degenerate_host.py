"""CPU: what tests/degenerate_cases.py claims about its cases, proved on the oracle alone -- conditions, not measurements.
tests/test_gpu_degenerate.py demands the oracle's BITS of the library on every solver path, which is only fair where the
oracle's own result does not depend on the order of its sums."""
import numpy as np
import pytest
import torch

import degenerate_cases as DC
from helpers import SumTap, same_bits, scalar_history

FAMILY_MESH = sorted({(c["family"], c["mesh"]) for c in DC.cases()})


def _group(family, mesh):
    return [c for c in DC.cases(family) if c["mesh"] == mesh]


def _same_float(a, b):
    return bool(same_bits(torch.tensor([a], dtype=torch.float64), torch.tensor([b], dtype=torch.float64)))


def test_the_table_covers_what_it_names():
    cs = DC.cases()
    assert {c["family"] for c in cs} == set("ABCD")
    for fam in "ABCD":
        assert {c["dtype"] for c in DC.cases(fam)} == {"single", "double"}, fam
        assert {c["method"] for c in DC.cases(fam)} == set(DC.METHODS), fam
    a = DC.cases("A")
    assert {c["mesh"] for c in a} == set(DC.A_MESHES) and {c["tol"] for c in a} == {1e-6, 0.0, -1.0}
    assert {c["bcname"] for c in a} == {"dir0", "mixed0", "periodic", "dir03"} and all(c["max_it"] == 5 for c in a)
    assert {(c["mesh"], c["max_it"]) for c in DC.cases("C")} == {(m, k) for m in ("c1", "c2", "c3") for k in range(5)}
    d = DC.cases("D")
    # the one-cell right-hand side visits every named place of the tiled meshes for chunks 1 and 2, and on the resident
    # mesh every index of the three centre lines, next to the neumann and the symmetry faces included
    from edge_fields import distinct_positions
    for mesh in ("t64", "t32"):
        n, dtype = DC.MESHES[mesh][0], DC.MESHES[mesh][1][0]
        want = {at for ch in (1, 2) for _, at in distinct_positions(n, dtype, ch)}
        for bcname in ("dir0", "mixed0"):
            assert {c["rhs"][1] for c in d if c["mesh"] == mesh and c["bcname"] == bcname} == want
    n = DC.MESHES["r3"][0]
    got = {c["rhs"][1] for c in d if c["mesh"] == "r3"}
    assert len(got) == sum(n) - 2 and all(sum(1 for q in range(3) if at[q] != n[q] // 2) <= 1 for at in got)
    for a_, (lo, hi) in enumerate(((1, n[0] - 2), (1, n[1] - 2), (1, n[2] - 2))):
        for i in (lo, hi):
            assert tuple(i if q == a_ else n[q] // 2 for q in range(3)) in got
    assert DC.MIXED0[1][0] == "neumann" and DC.MIXED0[2][0] == "symmetry" and DC.MIXED0[4][0] == "neumann"


def test_the_does_not_apply_list_is_explicit_and_short():
    pairs = [(c, p) for c in DC.cases() for p, _, _ in DC.paths_of(c)]
    na = [(c, p) for c, p in pairs if DC.not_applicable(c, p) is not None]
    assert na and 4 * len(na) <= len(pairs), (len(na), len(pairs))
    for _, path, reason in DC.NOT_APPLICABLE:
        assert isinstance(reason, str) and len(reason) > 20
        assert any(path in DC.PATHS[k] for k in DC.PATHS)
    for c in DC.cases():   # every case keeps at least three paths, the stepwise one for CG among them
        left = [p for p, _, _ in DC.paths_of(c) if DC.not_applicable(c, p) is None]
        assert len(left) >= 3 and (("stepwise" in left) == (c["method"] == "cg")), c["name"]


@pytest.mark.parametrize("family,mesh", FAMILY_MESH, ids=["%s-%s" % fm for fm in FAMILY_MESH])
def test_outcomes_are_the_pinned_ones(family, mesh):
    for c in _group(family, mesh):
        o, pin = DC.oracle(c), DC.pinned_outcome(c)
        if pin is None:
            assert family == "C"
            continue
        if pin == "raises":
            assert o["raised"] is not None and "Invalid tolerance" in o["raised"], (c["name"], o)
            continue
        assert o["raised"] is None, (c["name"], o["raised"])
        itr, tol, conv = pin
        assert (o["itr"], o["converge"]) == (itr, conv), (c["name"], o["itr"], o["converge"])
        if tol is not None:
            assert o["tol"] == tol, (c["name"], o["tol"])
        if family in "AB":   # x is the BC-filled x0
            import pyapes_oracle as O
            _, x0 = DC.inputs(c)
            O.bc_fill(x0, O.make_bcs(DC.oracle_mesh(c), DC.oracle_cfg(c)))
            assert same_bits(o["x"], x0), c["name"]


def test_one_unknown_outcomes_the_oracle_decides():
    """the figure the family was set up on: CG on 3^3 in fp32 raises from max_it = 2, and fp32 and fp64 differ"""
    got = {(c["dtype"], c["max_it"]): DC.oracle(c)["raised"] is not None
           for c in DC.cases("C") if c["mesh"] == "c3" and c["method"] == "cg"}
    assert [got[("single", k)] for k in range(5)] == [False, False, True, True, True]
    assert [got[("double", k)] for k in range(5)] != [got[("single", k)] for k in range(5)]
    raised = [c for c in DC.cases("C") if DC.oracle(c)["raised"] is not None]
    assert {c["method"] for c in raised} == {"cg", "bicgstab"} and {c["dtype"] for c in raised} == {"single", "double"}
    for c in raised:
        assert "Invalid tolerance" in DC.oracle(c)["raised"]


@pytest.mark.parametrize("family,mesh", FAMILY_MESH, ids=["%s-%s" % fm for fm in FAMILY_MESH])
def test_no_summation_order(family, mesh):
    """five summation orders of the oracle's dot products: identical bits in x, itr, tol and the raise ("all", "zero_den");
    family D's BiCGSTAB ("start"): identical r0.r0 and r0.v, itr and converge, x to rounding"""
    for c in _group(family, mesh):
        base = DC.oracle(c)
        for v in range(1, 5):
            tap = SumTap()
            o = DC.oracle_run(c, v, (tap,))
            assert (o["raised"] is None) == (base["raised"] is None), (c["name"], v)
            assert o["itr"] == base["itr"] and o["converge"] == base["converge"], (c["name"], v)
            if c["free"] == "start":
                assert _same_float(tap.vals[0], base["sums"][0]) and _same_float(tap.vals[1], base["sums"][1]), (c["name"], v)
                assert float((o["x"] - base["x"]).abs().max()) <= 1e-5 * float(base["x"].abs().max()), (c["name"], v)
                continue
            if base["raised"] is None:
                assert same_bits(o["x"], base["x"]), (c["name"], v, same_bits(o["x"], base["x"]))
                assert _same_float(o["tol"], base["tol"]), (c["name"], v, o["tol"], base["tol"])
            if c["free"] == "all":   # then every sum is the same number too
                assert len(tap.vals) == len(base["sums"]), (c["name"], v)
                skip = 3 if (family == "D" and c["method"] == "cg") else -1
                assert all(_same_float(a, b) for i, (a, b) in enumerate(zip(tap.vals, base["sums"])) if i != skip), (c["name"], v)


@pytest.mark.parametrize("family,mesh", FAMILY_MESH, ids=["%s-%s" % fm for fm in FAMILY_MESH])
def test_term_counts(family, mesh):
    """"all": every summed product has at most two finite non-zero terms, or a non-finite one (NaN whatever the order) --
    but for the r'.r' that closes family D's single CG iteration, which feeds the beta of an iteration that never comes.
    "zero_den": the first denominator (d.Ad; r0.v) is exactly zero with no non-zero term, the numerator is not.
    "start": r0.r0 and r0.v are one-term sums."""
    for c in _group(family, mesh):
        o = DC.oracle(c)
        terms, sums = o["terms"], o["sums"]
        assert len(terms) == len(sums)
        if c["method"] == "jacobi":
            assert not sums       # no dot product feeds a Jacobi iterate
            continue
        assert sums, c["name"]
        if c["free"] == "all":
            for i, (nz, nonfinite) in enumerate(terms):
                if family == "D" and c["method"] == "cg" and i == 3:
                    continue
                assert nz <= 2 or nonfinite > 0, (c["name"], i, terms)
        elif c["free"] == "zero_den":
            assert sums[0] != 0 and np.isfinite(sums[0]) and sums[1] == 0 and terms[1] == (0, 0), (c["name"], sums[:2], terms[:2])
        else:
            assert c["free"] == "start" and terms[0][0] <= 1 and terms[1][0] <= 1 and terms[0][1] == terms[1][1] == 0
        if family == "D" and c["method"] == "cg":
            assert terms[0][0] <= 1 and terms[1][0] <= 1 and terms[2][0] <= 1, (c["name"], terms)


@pytest.mark.parametrize("mesh", DC.A_MESHES)
def test_zero_start_is_exactly_zero(mesh):
    """family A: the residual the loops start from is zero at every node, the x0 = 0.3 case included (a row of the stencil
    times a constant: (c x - 2 c x) + c x, exact in any precision)"""
    for c in _group("A", mesh):
        r = DC.first_residual(c)
        assert not bool((r != 0).any()) and not bool(torch.isnan(r).any()), c["name"]
        o = DC.oracle(c)
        if c["method"] != "jacobi":
            assert o["sums"][0] == 0.0, (c["name"], o["sums"][:1])
    assert any(c["x0"] == ("const", 0.3) for c in _group("A", mesh))


def test_zero_denominators_of_family_b():
    seen = set()
    for c in DC.cases("B"):
        o = DC.oracle(c)
        if c["method"] == "jacobi":   # its denominator is diag(A)
            assert o["raised"] is not None
            continue
        assert o["sums"][1] == 0.0 and o["sums"][0] != 0.0, (c["name"], o["sums"][:2])
        assert o["scalars"]["alpha"] == 0.0
        seen.add(c["eq"])
    assert seen == {("lap", 0.0), ("lap", "zeros"), ("div", 0.6)}


def test_expected_scalars_restate_scalar_history():
    """the scalars demanded of the library against helpers.scalar_history on the same sums (fp64, where both form their
    quotients in doubles): every complete row, and what an incomplete last iteration leaves"""
    checked = 0
    for c in DC.cases():
        if c["dtype"] != "double" or c["method"] == "jacobi":
            continue
        o = DC.oracle(c)
        hist, exp = scalar_history(c["method"], o["sums"]), o["scalars"]
        if c["method"] == "cg" and len(o["sums"]) % 4 == 0 and len(hist):
            assert _same_float(hist[-1][0], exp["alpha"]) and _same_float(hist[-1][1], exp["beta"]), (c["name"], hist[-1], exp)
            assert exp["rr"] == o["sums"][-1] or (exp["rr"] != exp["rr"])
            checked += 1
        if c["method"] == "bicgstab" and len(hist) and (len(o["sums"]) - 1) % 4 == 0:
            a, om, rn = hist[-1]
            assert _same_float(a, exp["alpha"]) and _same_float(om, exp["omega"]) and _same_float(rn, exp["rho_next"]), (c["name"], hist[-1], exp)
            if o["raised"] is None:   # the look-ahead of pa_step_bicg_close: rho <- rho'
                assert _same_float(exp["rho"], exp["rho_next"])
            checked += 1
    assert checked > 100
    # a zero start that raises: alpha = 0/0 -> 0 twice, beta = 0/0 = NaN, and BiCGSTAB's rho' = -0 * 0 = -0.0
    c = next(c for c in DC.cases("A") if c["name"] == "A-g3d-dir0-cg-tol-1")
    s = DC.oracle(c)["scalars"]
    assert s["alpha"] == 0.0 and s["beta"] != s["beta"] and s["rr"] == 0.0
    c = next(c for c in DC.cases("A") if c["name"] == "A-g3d-dir0-bicgstab-tol-1")
    s = DC.oracle(c)["scalars"]
    assert s["alpha"] == 0.0 and s["beta"] != s["beta"] and s["omega"] == 0.0
    assert s["rho_next"] == 0.0 and np.signbit(s["rho_next"]) and np.signbit(s["rho"])
    c = next(c for c in DC.cases("A") if c["name"] == "A-g3d-dir0-bicgstab-tol0")
    s = DC.oracle(c)["scalars"]       # the first stop test ends the solve: omega is still the 1.0 it started with
    assert s == {"rr": 0.0, "r0v": 0.0, "alpha": 0.0, "omega": 1.0, "rho": 0.0, "rho_next": 0.0, "beta": 0.0}


def test_reuse_endings_exist():
    for ending in DC.REUSE_ENDINGS:
        cs = DC.reuse_cases(ending)
        assert {c["mesh"] for c in cs} == set(DC.REUSE_MESHES[ending]), ending
        for c in cs:
            o = DC.oracle(c)
            assert (o["raised"] is not None) == ending.endswith("raised"), (ending, c["name"])
            for m in DC.METHODS:
                f = DC.oracle(DC.follow_up(c, m))
                if c["family"] == "C":   # one unknown: no solve on it is an ordinary one; the comparison is what counts
                    continue
                assert f["raised"] is None and f["itr"] == 6 and f["tol"] > 0
