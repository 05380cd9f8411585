"""No GPU: every mesh of tests/grid_cap_cases.py has the property it is in the table for, proved from the restated launch
arithmetic alone, and the oracle returns a finite iterate with the iteration count asked for on every solver case
tests/test_gpu_grid_cap.py runs.  Each test counts what it checked."""
import math

import torch

import grid_cap_cases as C
import march_ref as R
import pyapes_oracle as O


def test_flat_meshes_take_more_than_one_pass():
    ran = 0
    for mid in C.FLAT:
        n, _ = C.MESHES[mid]
        assert C.cells(n) > C.PASS and C.trips(C.cells(n)) >= 2, mid
        ran += 1
    assert ran == 6
    n = C.MESHES["one_and_a_bit"][0]
    assert C.cells(n) == 533628 and C.cells(n) - C.PASS == 9340 and C.trips(C.cells(n)) == 2     # most threads one trip, some two
    for mid in C.PARTIAL_SECOND_TRIP:
        assert C.PASS < C.cells(C.MESHES[mid][0]) < 1.02 * C.PASS, mid
    n = C.MESHES["three_trips"][0]
    assert C.cells(n) == 1057500 and C.trips(C.cells(n)) == 3 and C.cells(n) - 2 * C.PASS > 0
    assert C.MESHES["line"][0] == [600001] and C.trips(600001) == 2
    n = C.MESHES["plane"][0]
    assert len(n) == 2 and n[1] % 2 == 1 and C.cells(n) == 525700
    for mid, lower in (("rz_plane", 0.0), ("rz_plane_off", 0.5)):
        om = C.omesh(mid, "double")
        assert om.coord == "rz" and float(om.grid[0].min()) == lower and C.trips(C.cells(om.nx)) == 2
    assert C.trips(C.LIMITER_N) == 2 and C.PASS < C.LIMITER_N


def test_big_shell_is_beyond_one_pass_and_between_the_path_thresholds():
    n = C.MESHES["big_shell"][0]
    assert C.shell_nodes(n) == 2 * (520 * 520 + 5 * 520 + 5 * 520) == 551200
    assert C.trips(C.shell_nodes(n)) == 2
    assert C.SHELL_PAIR < C.SHELL_FACES < C.shell_nodes(n) < C.SHELL_ONE_PASS
    assert C.trips(C.cells(n)) == 3
    # the other flat meshes keep their shell within one pass: the shell trips are this mesh's alone
    assert all(C.trips(C.shell_nodes(C.MESHES[m][0])) == 1 for m in C.FLAT)
    assert C.shell_nodes([700, 751]) == 2 * (700 + 751) and C.shell_nodes([600001]) == 2


def test_tile_counts_predicted_for_the_tiled_meshes():
    """16-row tiles (pick_rj gives 4 rows per thread to a 2-D mesh, and to a 3-D one whose chunks stay shorter than 24
    planes whatever the tile height)"""
    ran = 0
    for mid, (dtype, options, layout) in C.TILED.items():
        n, _ = C.MESHES[mid]
        assert C.layout_of(n, dtype, bool(options.get("pitch", 1))) == layout, mid
        per = C.upper_periodic(mid, "dn")
        assert per == (False, False)
        inner, full = C.tiles(n, dtype, layout, True, upper_periodic=per), C.tiles(n, dtype, layout, False, upper_periodic=per)
        if mid == "tiles_straddle":
            assert (inner, full) == (32 * 64, 33 * 65) and inner <= C.PA_MAX_GRID < full
        else:
            assert inner == 33 * 65 == 2145 and full >= inner > C.PA_MAX_GRID, (mid, inner, full)
        assert full <= C.PA_MAX_PARTIALS
        ran += 1
    assert ran == 5
    assert C.tile_count(513, 4097, 4, 1) == 2145 and C.tile_count(512, 4096, 4, 1) == 2048
    assert C.tile_count(528, 8320, 4, 2) == 2145 and C.tile_count(527, 8319, 4, 2) == 2145
    # tiles_above_3d: axis 0 is shorter than 24 planes, so both candidate tile heights leave short chunks and pick_rj keeps 4;
    # more tiles than any capacity of 256 CUs x at most 8 blocks gives one chunk: blocks = tiles
    n = C.MESHES["tiles_above_3d"][0]
    assert n[0] < 24 and C.tiles(n, "single", "narrow", True) > 256 * 8
    # the 2-D tiled meshes are above k_cg2d's default threshold (1.5 M cells): the tests switch it off to reach k_cg3d
    assert all(C.cells(C.MESHES[m][0]) >= 1500000 for m in C.TILED if len(C.MESHES[m][0]) == 2)


def test_solver_cases_have_a_dirichlet_face_and_a_finite_oracle_iterate():
    ran = 0
    for case in C.SOLVES:
        mid, dtype, bc, method, iters = case
        _, ocfg = C.solve_cfgs(case, "cpu")
        types = [c["bc_type"] for c in ocfg]
        assert "dirichlet" in types and not all(t == "periodic" for t in types), case
        assert dtype == "double" or "periodic" not in types, case
        x, rep = C.oracle_solution(case)
        assert rep["itr"] == iters, (case, rep)
        assert x.dtype == C.tdtype(dtype) and bool(torch.isfinite(x).all()), case
        assert math.isfinite(rep["tol"]) and rep["tol"] > 0.0, (case, rep)
        ran += 1
    assert ran == len(C.SOLVES) == 27 + 8 + 20
    assert {c[0] for c in C.TILED_SOLVES} == set(C.TILED) and {c[0] for c in C.SHELL_SOLVES} == {"big_shell"}
    # the shell solves reach each default BC path: closed form (pairable, no periodic face), pair kernels (a periodic axis,
    # above 150 k shell nodes), one launch per face (listed out of the factory order)
    assert {c[2] for c in C.SHELL_SOLVES} == {"mix", "xper", "mix_shuffled"}
    assert [c["bc_face"] for c in C.bc_lists("big_shell", "double", "mix_shuffled", device="cpu")[1]] == ["yl", "yu", "xl", "xu", "zl", "zu"]
    assert C.faces_of("big_shell", "xper")[0][0] == C.faces_of("big_shell", "xper")[1][0] == "periodic"
    assert {"one_and_a_bit", "line", "plane", "rz_plane"} <= {c[0] for c in C.GENERIC_SOLVES}
    assert {(c[0], c[1]) for c in C.GENERIC_SOLVES} >= {("one_and_a_bit", "double"), ("one_and_a_bit", "single")}


def test_general_upwind_restatement_is_the_marches_statement():
    """grid_cap_cases.div_general_upwind: on a scalar target it is march_ref.adv_upwind and the oracle's intended upwind; on a
    vector target each axis reads its own component and its own speed"""
    om = O.OMesh([0.0, 0.0, 0.0], [1.0, 1.1, 0.5], [6, 7, 9], "single")
    g = torch.Generator().manual_seed(3)
    phi = torch.randn((1, 6, 7, 9), generator=g, dtype=torch.float64).float()
    V = torch.randn((3, 6, 7, 9), generator=g, dtype=torch.float64).float()
    U = torch.randn((3, 6, 7, 9), generator=g, dtype=torch.float64).float()
    assert torch.equal(C.div_general_upwind(0.7, phi, om), O.div_upwind_intended(0.7, phi, om))
    assert torch.equal(C.div_general_upwind(U[:1], phi, om), R.adv_upwind([U[0]] * 3, phi, om))
    assert torch.equal(C.div_general_upwind(U, V, om), O.div_upwind_intended(U, V, om))
    want = sum(R.adv_upwind([U[a] if b == a else 0.0 for b in range(3)], V[a:a + 1], om) for a in range(3))
    assert torch.allclose(C.div_general_upwind(U, V, om), want, rtol=1e-5, atol=1e-5)
    assert not torch.equal(C.div_general_upwind(U, V, om), C.div_general_upwind(U, V[[1, 0, 2]], om))
    # on a cylinder: the oracle's intended upwind up to the order of the last two additions, and the r term is there
    rz = O.OMesh([0.5, 0.0], [1.5, 1.5], [9, 11], "double", "rz")
    p2 = torch.randn((1, 9, 11), generator=g, dtype=torch.float64)
    u2 = torch.randn((1, 9, 11), generator=g, dtype=torch.float64)
    got, want = C.div_general_upwind(u2, p2, rz), O.div_upwind_intended(u2, p2, rz)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    flat = O.OMesh([0.5, 0.0], [1.5, 1.5], [9, 11], "double")
    assert float((got - C.div_general_upwind(u2, p2, flat)).abs().max()) > 1e-3


def test_limiter_operands_cover_the_pass_boundary():
    for dtype in ("double", "single"):
        a, b = C.limiter_operands(dtype)
        assert a.numel() == b.numel() == C.LIMITER_N
        assert float(a[C.PASS - 1]) == -float(b[C.PASS - 1]) != 0.0 and bool(torch.isnan(a[C.PASS])) and float(b[C.PASS]) == 1.0
        for sl in (slice(0, 144), slice(C.PASS - 72, C.PASS + 72), slice(C.LIMITER_N - 144, None)):
            for t in (a[sl], b[sl]):
                assert bool(torch.isnan(t).any()) and bool(torch.isinf(t).any()) and bool((t == 0).any())
                assert bool(torch.signbit(t[t == 0]).any()) and not bool(torch.signbit(t[t == 0]).all())
                tiny = torch.finfo(t.dtype).tiny
                assert bool(((t.abs() > 0) & (t.abs() < tiny)).any())           # denormals
        m = O.minmod(a, b)
        assert bool(torch.isfinite(m[torch.isfinite(a) & torch.isfinite(b)]).all())
