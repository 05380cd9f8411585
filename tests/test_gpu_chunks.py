"""-m gpu: the marching kernels on chunks LONGER THAN ONE PLANE (k_sf, k_sfq, the 3-D phases of k_cg3d).

The launchers size their axis-0 chunks as  chunks = min(n0, CUs * blocks_per_CU / tiles).  On a 256-CU part that is at least
512 blocks for the 1 .. 10 tiles of every small mesh of this suite: chunks == n0, every workgroup marches exactly ONE plane,
only the first of the four unrolled copies of the plane loop runs, the register slots never change roles and the clamp at
the chunk end applies to every plane.  Option "chunks" N caps the chunk count behind the rule and option "sf" 2 / 4 forces
the rows per wave of k_sf (as "sfq" 2 / 4 does for k_sfq), so that small meshes reach the rest of the plane loop.

Every check has two yardsticks, neither of which is the code under test:
  * the generic kernels (option "fastpath" 0: one thread per node, no chunks), bit for bit (helpers.bit_equal) -- every
    tiled launch is compared with them;
  * the CPU references, each with the criterion the suite already uses for that scheme: QUICK tests/march_ref.py bit for bit
    (test_gpu_quick.py), central pyapes_oracle.euler_step bit for bit (test_gpu_parity_golden.py), intended upwind
    pyapes_oracle.euler_step to rel_err 1e-13 (fp64) / 1e-6 (fp32) (test_gpu_fuzz.py); a stage is c0 * phi0 + c1 * E in the
    mesh dtype followed by the oracle's bc_fill.  (The literal "compat" upwind has no CPU statement in the oracle's Euler
    step: the generic kernels alone.)  The generic result is held against the CPU reference once per case; a tiled
    launch that equals the generic bits then meets the same criterion with the same figures.
"""
import random
import re
import sys
import warnings

import pytest
import torch

import march_gpu as G
import march_ref as Q
import pyapes_oracle as O
import test_gpu_fuzz as F
import test_gpu_quick as TQ
import test_gpu_rk as R
import test_self_march_host as HS
from helpers import bit_equal, hip_options, rel_err
from pyapes_amd.geometry import Box
from pyapes_amd.hip.context import context_for
from pyapes_amd.mesh import Mesh
from pyapes_amd.solver.fdc import FDC, div_kind
from pyapes_amd.solver.fdm import FDM
from pyapes_amd.solver.march import euler_march, rk_march
from pyapes_amd.solver.ops import Solver
from pyapes_amd.variables import Field

pytestmark = pytest.mark.gpu

UPWIND, COMPAT, CENTRAL, QUICK = R.UPWIND, R.COMPAT, R.CENTRAL, TQ.QUICK
CONFIG = {"upwind": UPWIND, "compat": COMPAT, "central": CENTRAL, "quick": QUICK}
LIMITER = {"upwind": "upwind", "central": "none"}
XPER = TQ.XPER
ALLPER = ([None] * 6, ["periodic"] * 6)
BCNAME = {id(R.NEUSYM): "NEUSYM", id(R.ALLNEU): "ALLNEU", id(R.MIXED): "MIXED", id(R.ALLDIR): "ALLDIR", id(R.YPER): "YPER",
          id(R.DIRPER): "DIRPER", id(XPER): "XPER", id(ALLPER): "ALLPER"}
CAPS = (1, 2, 3, 5, 0)                      # 0: the rule alone (one plane per chunk on these meshes)
STAGES = [None, R.ALL4[0], R.ALL4[1]]       # the Euler step and two (c0, c1) pairs
DTYPES = ["double", "single"]


def _kind(scheme):
    cfg = CONFIG[scheme]["div"]
    return div_kind(cfg["limiter"], bool(cfg.get("compat", False)))


def _n2(n2, dtype):
    """rows are whole 16-byte vectors on the tiled kernels: 34 stays 34 in fp64 and becomes 36 in fp32"""
    v = 2 if dtype == "double" else 4
    return (n2 + v - 1) // v * v


class Case:
    """one mesh with BC-filled fields (phi_s, phi0), a randn speed field, the oracle's mesh and BCs, BCs bound in the context"""

    def __init__(self, n, dtype, bcs, seed=17):
        key = "_chunks_case"
        R.CASE[key] = (key, list(n), dtype, bcs, UPWIND, "field", False, {}, "")
        try:
            self.mesh, self.bc, _, self.phis, self.phi0, self.ufield, self.nu, self.dt = R._setup(key, seed)
        finally:
            del R.CASE[key]
        self.n, self.dtype, self.bcs = list(n), dtype, bcs
        self.om = O.OMesh([0.0] * 3, [1.0] * 3, list(n), dtype)
        self.ob = O.make_bcs(self.om, O.mixed_cfg(list(bcs[0]), list(bcs[1]), O.FACES[:6]))
        self.ctx = context_for(self.mesh)
        self.rebind()
        self.tag = ("x".join(map(str, n)), dtype, BCNAME.get(id(bcs), bcs[1]))

    def rebind(self):
        f = G.fresh_field(self.mesh, self.bc, self.phis)
        self.ctx.bind_bcs(f(), f.bcs, 0)

    def options(self, **kw):
        for k, v in kw.items():
            self.ctx.set_option(k, v)

    def generic(self):
        self.options(fastpath=0, chunks=0, sf=1, sfq=1)

    def tiled(self, cap, rows=0, sf=None):
        self.options(fastpath=1, chunks=cap, sf=(rows or 1) if sf is None else sf, sfq=rows or 1)

    def speed(self, form):
        return {"pos": 1.3, "neg": -0.8, "zero": 0.0, "field": self.ufield, "self": self.phis}[form]

    def launch(self, scheme, form, stage, source=None, velocity=None):
        """one Euler step (stage None) or fused stage; source: None, a number or a tensor of one component's shape; velocity:
        None, or one entry per axis in place of the speed `form` names (tests/test_gpu_chunks_terms.py)"""
        out = torch.full_like(self.phis, float("nan"))
        if velocity is not None:
            if stage is None:
                self.ctx.euler_step_vel(self.phis[0], out[0], _kind(scheme), velocity, self.nu, self.dt, source=source)
            else:
                self.ctx.rk_stage_vel(self.phis[0], self.phi0[0], out[0], stage[0], stage[1], _kind(scheme), velocity, self.nu, self.dt,
                                      source=source)
            return out
        u = self.speed(form)
        if stage is None:
            self.ctx.euler_step(self.phis[0], out[0], _kind(scheme), u, self.nu, self.dt, source=source)
        else:
            self.ctx.rk_stage(self.phis[0], self.phi0[0], out[0], stage[0], stage[1], _kind(scheme), u, self.nu, self.dt, source=source)
        return out

    def cpu(self, scheme, form, stage):
        """the CPU reference of launch(), None where the suite has none (compat)"""
        x = self.phis.cpu().clone()
        u = self.speed(form)
        uc = x if form == "self" else (u.cpu().clone() if isinstance(u, torch.Tensor) else u)
        if scheme == "quick":
            e = Q.euler_step(x, uc, self.nu, self.dt, self.om, self.ob, "quick")
        elif scheme in LIMITER:
            e = O.euler_step(x, uc, self.nu, self.dt, self.om, self.ob, LIMITER[scheme])
        else:
            return None
        if stage is None:
            return e
        out = (stage[0] * self.phi0.cpu()) + (stage[1] * e)
        assert out.dtype == x.dtype
        O.bc_fill(out, self.ob)
        return out


def meets(scheme, dtype, got, ref):
    """(ok, figure): the suite's criterion for that scheme"""
    if scheme == "upwind":
        e = rel_err(got.cpu(), ref)
        return e <= (1e-13 if dtype == "double" else 1e-6), e
    return bit_equal(got, ref), int((got.cpu() != ref).sum())


def told(bad, show):
    """the failing cases' parameters, as one string (a tuple's repr is cut short in the report)"""
    return "%d differ; the first: %s" % (len(bad), " | ".join(repr(b) for b in bad[:show]))


def where(a, b):
    """(cells that differ, axis-0 planes that hold them)"""
    d = a != b
    d = d.movedim(-3, 0).reshape(d.shape[-3], -1)
    return int(d.sum()), d.any(1).nonzero().flatten().tolist()[:8]


# ---- the meshes of (b): n0 from {5, 6, 7, 9, 13, 18}, n1 x n2 the shapes the existing tables justify ------------------------
def step_meshes(dtype, scheme, kernel):
    big = (20, 136) if dtype == "double" else (40, 264)       # two k tiles: the edge-cell pairs
    a = _n2(34, dtype)
    if scheme == "central":   # (central Div is refused on neumann / symmetry faces)
        ms = [([9, 5, 32], R.ALLDIR), ([13, 19, a], R.ALLDIR), ([13, *big], R.ALLDIR), ([18, 4, 32], R.ALLDIR), ([5, 36, 72], R.ALLDIR),
              ([7, 6, 32], R.ALLDIR), ([6, 19, a], R.ALLDIR), ([9, 6, 32], R.DIRPER), ([13, 19, a], XPER), ([6, 6, 32], ALLPER)]
    else:
        ms = [([5, 19, a], R.MIXED), ([6, 36, 72], R.NEUSYM), ([7, 6, 32], R.ALLNEU), ([9, 5, 32], R.ALLDIR), ([13, 19, a], R.ALLDIR),
              ([18, 4, 32], R.MIXED), ([13, *big], R.ALLDIR), ([7, 19, a], R.YPER), ([9, 6, 32], R.DIRPER), ([18, 36, 72], R.MIXED),
              ([13, 19, a], XPER), ([6, 6, 32], ALLPER)]
    if kernel == "k_sfq":     # five nodes per axis at least, and k_sfq declines a periodic axis 0 (asserted in the child of (a))
        ms = [m for m in ms if m[0][1] >= 5 and m[1][1][0] != "periodic"]
    return ms


def sweep_steps(dtype, scheme, form, meshes, rows_list, sf=None):
    """every mesh x stage x rows x cap: tiled == generic in every bit, generic meets the CPU criterion"""
    bad, launches = [], 0
    for n, bcs in meshes:
        c = Case(n, dtype, bcs)
        c.generic()
        gen = [c.launch(scheme, form, st) for st in STAGES]
        for st, g in zip(STAGES, gen):
            assert bool(torch.isfinite(g).all())
            ref = c.cpu(scheme, form, st)
            if ref is not None:
                ok, fig = meets(scheme, dtype, g, ref)
                if not ok:
                    bad.append((c.tag, scheme, form, "generic vs CPU", st, fig))
        for rows in rows_list:
            if rows == 4 and sf is None and scheme != "quick" and n[1] <= 8:
                continue                      # k_sf: the one- and two-row rules stand in front of the forced value
            for cap in CAPS:
                c.tiled(cap, rows, sf)
                for st, g in zip(STAGES, gen):
                    out = c.launch(scheme, form, st)
                    launches += 1
                    if not bit_equal(out, g):
                        bad.append((c.tag, scheme, form, "rows", rows, "cap", cap, "stage", st, where(out, g)))
    assert not bad, told(bad, 6)
    return launches


# ---- (a) the switches do what they say ---------------------------------------------------------------------------------------
def _mark(tag):
    torch.cuda.synchronize()
    sys.stderr.write("CASE %s\n" % tag)
    sys.stderr.flush()


def _by_case(log):
    return G.case_log(log, lambda ln: "[pyapes_hip]" in ln)


def _field_of(line, word):
    """the integer behind `word` in a launch line ("chunks 2", "RJ 4", "(CI ~6")"""
    return int(re.search(re.escape(word) + r"(\d+)", line).group(1))


def switch_child():
    """(a) in the child process: launches whose log lines the parent reads"""
    c = Case([13, 20, 36], "double", R.ALLDIR)
    for cap in (0, 3, 1000):
        c.tiled(cap)
        _mark("sf cap %d" % cap)
        c.launch("upwind", "field", None)
        _mark("sfq cap %d" % cap)
        c.launch("quick", "field", None)
        c.tiled(cap, sf=0)
        _mark("cg3d cap %d" % cap)
        c.launch("upwind", "field", None)
    for rows, n1 in ((4, 20), (4, 6), (2, 20)):
        d = Case([7, n1, 32], "double", R.ALLDIR)
        d.tiled(2, rows)
        _mark("rows %d n1 %d" % (rows, n1))
        d.launch("central", "pos", None)
    x = Case([13, 20, 36], "double", XPER)            # k_sfq declines a periodic axis 0: the generic step, k_sf for upwind
    x.tiled(2)
    _mark("xper quick")
    x.launch("quick", "pos", R.ALL4[0])
    _mark("xper upwind")
    x.launch("upwind", "pos", None)
    # the first cases of the seeded sweep (d): taken by the tiled kernel, chunks of two planes or more
    for k, p in enumerate(sweep_cases(24)):
        assert run_sweep_case(p, lambda: _mark("sweep %d" % k)) is None, p
        _mark("-")
    torch.cuda.synchronize()


def test_switches_do_what_they_say():
    log = G.child("import torch\nimport test_gpu_chunks as T\nT.switch_child()\n", drop_options=True)
    seen = _by_case(log)
    for kern, word in (("sf", "k_sf "), ("sfq", "k_sfq "), ("cg3d", "k_cg3d ")):
        rule = [ln for ln in seen["%s cap 0" % kern] if word in ln]
        capd = [ln for ln in seen["%s cap 3" % kern] if word in ln]
        high = [ln for ln in seen["%s cap 1000" % kern] if word in ln]
        assert len(rule) == len(capd) == len(high) == 1, (kern, seen)
        assert _field_of(rule[0], "chunks ") == 13 and _field_of(rule[0], "(CI ~") == 1, rule    # the one-plane fact
        assert _field_of(capd[0], "chunks ") == 3 and _field_of(capd[0], "(CI ~") == 4, capd
        assert high[0] == rule[0], (high, rule)                                                  # a cap above the rule: nothing
    for tag, rj in (("rows 4 n1 20", 4), ("rows 4 n1 6", 2), ("rows 2 n1 20", 2)):
        ln = [ln for ln in seen[tag] if "k_sf " in ln]
        assert len(ln) == 1 and _field_of(ln[0], " RJ ") == rj and _field_of(ln[0], "chunks ") == 2, (tag, seen[tag])
    # (a periodic face: the stage is the step kernel + the combine kernel; the generic step itself has no log line)
    assert not any("k_sfq" in ln or "k_sf " in ln for ln in seen["xper quick"]) and any("k_rk_combine" in ln for ln in seen["xper quick"]), seen["xper quick"]
    assert any("k_sf " in ln and "chunks 2" in ln for ln in seen["xper upwind"]), seen["xper upwind"]
    for k, p in enumerate(sweep_cases(24)):
        lines = [ln for ln in seen["sweep %d" % k] if "k_sf " in ln or "k_sfq " in ln]
        assert len(lines) == 1, (p, seen["sweep %d" % k])
        assert ("k_sfq " in lines[0]) == (p["scheme"] == "quick"), (p, lines)
        assert _field_of(lines[0], "(CI ~") >= 2 and _field_of(lines[0], "chunks ") == p["cap"], (p, lines)
        assert ("(RK stage)" in lines[0]) == (p["stage"] is not None and "periodic" not in p["bcs"][1]), (p, lines)
        assert not any("k_euler" in ln or "k_cg3d" in ln for ln in seen["sweep %d" % k]), (p, seen["sweep %d" % k])


def test_options_round_trip():
    mesh = Mesh(Box[0:1, 0:1, 0:1], None, [7, 6, 32], "cuda", "double")
    ctx = context_for(mesh)
    assert ctx.get_option("chunks") == 0 and ctx.get_option("sf") == 1
    for v in (1, 2, 3, 5, 1000, 0):
        ctx.set_option("chunks", v)
        assert ctx.get_option("chunks") == v
    ctx.set_option("chunks", -4)
    assert ctx.get_option("chunks") == 0
    for v, back in ((0, 0), (1, 1), (2, 2), (4, 4), (3, 1), (7, 1), (1, 1)):
        ctx.set_option("sf", v)
        assert ctx.get_option("sf") == back


def test_options_come_from_the_environment(monkeypatch):
    hip_options(monkeypatch, chunks=3, sf=4)
    ctx = context_for(Mesh(Box[0:1, 0:1, 0:1], None, [7, 6, 32], "cuda", "double"))
    assert ctx.get_option("chunks") == 3 and ctx.get_option("sf") == 4
    hip_options(monkeypatch, chunks=None, sf=None)


# ---- (b) step and stage across chunk lengths ---------------------------------------------------------------------------------
SF_INSTANTIATIONS = [("upwind", "pos"), ("upwind", "neg"), ("upwind", "zero"), ("upwind", "field"), ("compat", "field"),
                     ("central", "pos"), ("upwind", "self"), ("central", "self")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme,form", SF_INSTANTIATIONS, ids=lambda v: v)
def test_k_sf_step_and_stage(scheme, form, dtype):
    assert sweep_steps(dtype, scheme, form, step_meshes(dtype, scheme, "k_sf"), (2, 4)) > 200


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["pos", "neg", "field", "self"])
def test_k_sfq_step_and_stage(form, dtype):
    assert sweep_steps(dtype, "quick", form, step_meshes(dtype, "quick", "k_sfq"), (2, 4)) > 200


def cg3d_meshes(dtype, scheme):
    a = _n2(34, dtype)
    mixed = R.ALLDIR if scheme == "central" else R.MIXED
    neusym = R.ALLDIR if scheme == "central" else R.NEUSYM
    # through "sf" 0 (whole vectors, k_cg3d's vector layout) and through an odd row length (one cell per lane)
    return [([13, 19, a], mixed), ([7, 36, 72], neusym), ([18, 6, 32], R.ALLDIR), ([9, 20, 136], R.DIRPER),
            ([13, 17, 35], mixed), ([9, 19, 33], R.ALLDIR), ([6, 13, 17], neusym), ([5, 7, 131], mixed)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme,form", [("upwind", "pos"), ("upwind", "neg"), ("upwind", "field"), ("compat", "field"),
                                         ("central", "pos"), ("upwind", "self")], ids=lambda v: v)
def test_k_cg3d_step_and_stage(scheme, form, dtype):
    assert sweep_steps(dtype, scheme, form, cg3d_meshes(dtype, scheme), (0,), sf=0) > 100


@pytest.mark.parametrize("dtype", DTYPES)
def test_div_term_alone(dtype):
    """FDC.div on k_sf phase 2: the generic kernels bit for bit; QUICK (generic on every path) == tests/march_ref.py"""
    bad = []
    for n, bcs in step_meshes(dtype, "upwind", "k_sf"):
        c = Case(n, dtype, bcs)
        central_ok = all(t in ("dirichlet", "periodic") for t in bcs[1])
        for scheme in ("upwind", "compat") + (("central",) if central_ok else ()):
            for form in ("pos", "neg", "field"):
                u = c.speed(form)
                cfg = {"div": dict(CONFIG[scheme]["div"], edge=False)}
                c.generic()
                gen = FDC(cfg).div(u, G.fresh_field(c.mesh, c.bc, c.phis)).clone()
                assert bool(torch.isfinite(gen).all())
                for rows in (2, 4):
                    for cap in CAPS:
                        c.tiled(cap, rows)
                        out = FDC(cfg).div(u, G.fresh_field(c.mesh, c.bc, c.phis))
                        if not bit_equal(out, gen):
                            bad.append((c.tag, scheme, form, rows, cap, where(out, gen)))
        if n[1] >= 5:
            c.tiled(2)
            out = FDC(QUICK).div(c.ufield, G.fresh_field(c.mesh, c.bc, c.phis))
            if not bit_equal(out, Q.div_quick(c.ufield.cpu(), c.phis.cpu(), c.om, c.ob)):
                bad.append((c.tag, "quick div"))
    assert not bad, told(bad, 6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_cg3d_laplacian_aop_gradient(dtype):
    """the explicit Laplacian (== the oracle bit for bit, the criterion of test_gpu_fuzz.py), A x and the gradient: the generic
    kernels bit for bit under every cap"""
    bad = []
    for n, bcs in cg3d_meshes(dtype, "upwind") + [([13, 19, _n2(34, dtype)], XPER), ([6, 6, 32], ALLPER)]:
        c = Case(n, dtype, bcs)

        def ops():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                var = G.fresh_field(c.mesh, c.bc, c.phis)
                solver = Solver({"fdm": {"method": "cg", "tol": 1e-6, "max_it": 1, "report": False}})
                solver.set_eq(-FDM().laplacian(0.7, var) == torch.zeros_like(var()))
                return {"lap": FDC({"laplacian": {"edge": False}}).laplacian(var).clone(), "aop": solver.Aop(var).clone(),
                        "grad": FDC({"grad": {"edge": False}}).grad(var).clone()}
        c.generic()
        gen = ops()
        x = c.phis.cpu().clone()
        lap_o = O.apply_laplacian(O.laplacian_tables(x, c.om, c.ob), x, 3)
        if not bit_equal(gen["lap"], lap_o):
            bad.append((c.tag, "generic Laplacian vs oracle"))
        for cap in CAPS:
            c.tiled(cap)
            for k, v in ops().items():
                if not bit_equal(v, gen[k]):
                    bad.append((c.tag, k, cap, where(v, gen[k])))
    assert not bad, told(bad, 6)


@pytest.mark.parametrize("dtype", DTYPES)
def test_k_cg3d_jacobi_three_sweeps(dtype):
    """three sweeps with "jac_alt" 1 (max_it 2): forwards, backwards (phase 9), forwards.  The iterate equals the generic
    kernels' bit for bit (the criterion of test_gpu_tiled_ops.py) and the oracle's to the tolerance of test_gpu_fuzz.py,
    with its iteration count"""
    tol = 1e-10 if dtype == "double" else 2e-5
    a = _n2(34, dtype)
    bad = []
    for n, bcs in [([13, 19, a], R.MIXED), ([7, 36, 72], R.ALLDIR), ([18, 6, 32], R.MIXED), ([9, 19, 33], R.ALLDIR), ([13, 17, 35], R.MIXED),
                   ([13, 19, a], XPER)]:
        g = torch.Generator().manual_seed(23)
        tdt = torch.float64 if dtype == "double" else torch.float32
        rhs0 = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        x0 = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        mesh = Mesh(Box[0:1, 0:1, 0:1], None, list(n), "cuda", dtype)
        ctx = context_for(mesh)
        bc = {"domain": R.mixed_bcs(*bcs), "obstacle": None}
        om = O.OMesh([0.0] * 3, [1.0] * 3, list(n), dtype)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            xo, ro = O.solve_poisson(om, O.mixed_cfg(list(bcs[0]), list(bcs[1]), O.FACES[:6]), rhs0.clone(), x0=x0.clone(), method="jacobi",
                                     tol=-1.0, max_it=2, coeff=0.8, sign=-1.0)

        def run(**opts):
            for k, v in dict(resident=0, jac_alt=1, **opts).items():
                ctx.set_option(k, v)
            var = Field("p", 1, mesh, bc)
            var.set_var_tensor(x0.cuda().clone())
            s = Solver({"fdm": {"method": "jacobi", "tol": -1.0, "max_it": 2, "report": False}})
            s.set_eq(-FDM().laplacian(0.8, var) == rhs0.cuda().clone())
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                rep = s.solve()
            return var().clone(), rep
        xg, rg = run(fastpath=0, chunks=0)
        if rg["itr"] != ro["itr"] or rel_err(xg.cpu(), xo) > tol:
            bad.append((n, "generic vs oracle", rg["itr"], ro["itr"], rel_err(xg.cpu(), xo)))
        for cap in CAPS:
            xt, rt = run(fastpath=1, chunks=cap)
            if rt["itr"] != ro["itr"] or not bit_equal(xt, xg):
                bad.append((n, BCNAME[id(bcs)], cap, rt["itr"], where(xt, xg)))
    assert not bad, told(bad, 6)


# ---- (c) marches: the BC-on-load patch of the plane behind / ahead meets a rotating slot -------------------------------------
MARCH_BCS = [R.NEUSYM, R.ALLNEU, R.MIXED, R.ALLDIR]


def march_meshes(dtype):
    # BC on load needs (n1 - 1) % rows != 0: 36 and 20 rows at two and four rows per wave, 6 rows at two; 19 rows decline it at two
    return [[7, 36, 72], [13, 20, 36], [13, 6, 32], [7, 19, _n2(34, dtype)]]


def _march(c, scheme, self_adv, order, u=None):
    f = G.fresh_field(c.mesh, c.bc, c.phis)
    if order == 0:
        return euler_march(f, f if self_adv else u, c.nu, c.dt, 3, CONFIG[scheme])().clone()
    return rk_march(f, f if self_adv else u, c.nu, c.dt, 3, CONFIG[scheme], order=order)().clone()


def _cpu_march(c, scheme, self_adv, order, u=None):
    x = c.phis.cpu().clone()
    uc = u.cpu().clone() if isinstance(u, torch.Tensor) else u
    order = order or 1
    if scheme == "quick":
        return Q.march(x, uc, c.nu, c.dt, 3, c.om, c.ob, "quick", order, self_adv=self_adv)
    if self_adv:
        return HS.oracle_self_march(x, c.nu, c.dt, 3, c.om, c.ob, LIMITER[scheme], order)
    return Q.march(x, uc, c.nu, c.dt, 3, c.om, c.ob, LIMITER[scheme], order, step=O.euler_step)


def sweep_marches(dtype, scheme, self_adv, orders, bcsets, speeds=("pos",), bcl=(1,)):
    bad, launches = [], 0
    for n in march_meshes(dtype):
        if scheme == "quick" and n[1] < 5:
            continue
        for bcs in bcsets:
            c = Case(n, dtype, bcs)
            for form in speeds:
                u = None if self_adv else c.speed(form)
                for order in orders:   # 0: euler_march
                    c.generic()
                    gen = _march(c, scheme, self_adv, order, u)
                    assert bool(torch.isfinite(gen).all())
                    ok, fig = meets(scheme, dtype, gen, _cpu_march(c, scheme, self_adv, order, u))
                    if not ok:
                        bad.append((c.tag, scheme, form, order, "generic vs CPU", fig))
                    for b in bcl:
                        for rows in (0, 4):
                            if rows == 4 and scheme != "quick" and n[1] <= 8:
                                continue
                            for cap in (1, 2, 3):
                                c.tiled(cap, rows)
                                c.options(bcl=b)
                                out = _march(c, scheme, self_adv, order, u)
                                launches += 1
                                if not bit_equal(out, gen):
                                    bad.append((c.tag, scheme, form, "order", order, "bcl", b, "rows", rows, "cap", cap, where(out, gen)))
    assert not bad, told(bad, 6)
    return launches


@pytest.mark.parametrize("dtype", DTYPES)
def test_euler_march_frozen_speed(dtype):
    """euler_march, upwind, "bcl" 1 and 0, the four non-periodic BC sets, scalar speeds of both signs and a speed field"""
    assert sweep_marches(dtype, "upwind", False, (0,), MARCH_BCS, ("pos", "neg", "field"), bcl=(1, 0)) > 200


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", ["upwind", "central", "quick"])
def test_rk_march_frozen_speed(scheme, dtype):
    bcsets = [R.ALLDIR] if scheme == "central" else MARCH_BCS
    assert sweep_marches(dtype, scheme, False, (2, 3), bcsets, ("pos",) if scheme == "central" else ("neg", "field")) > 40


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", ["upwind", "central", "quick"])
def test_rk_march_self_advected(scheme, dtype):
    bcsets = [R.ALLDIR] if scheme == "central" else MARCH_BCS
    assert sweep_marches(dtype, scheme, True, (3,) if scheme == "upwind" else (2, 3), bcsets) > 20


# ---- (d) a seeded sweep ---------------------------------------------------------------------------------------------------
def sweep_cases(count, seed=20261018):
    """every case is one the tiled kernel takes BY CONSTRUCTION: 3-D, five nodes or more per axis, rows of at least two
    whole vectors, a scalar BC on all six faces, aligned operands; central Div on dirichlet / periodic faces only, QUICK
    without a periodic axis 0; the cap leaves chunks of two planes or more"""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        dtype = rng.choice(DTYPES)
        scheme = rng.choice(["upwind", "upwind", "compat", "central", "quick", "quick"])
        n0, n1 = rng.randint(5, 23), rng.randint(5, 40)
        n2 = _n2(rng.choice([8, 12, 34, 64, 72, 132, 136, 260, 264]), dtype)
        types, vals = [], []
        for a in range(3):
            if rng.random() < 0.2:
                types += ["periodic", "periodic"]
                vals += [None, None]
            else:
                for _ in range(2):
                    t = rng.choice(["dirichlet", "dirichlet", "neumann", "symmetry"])
                    types.append(t)
                    vals.append(None if t == "symmetry" else round(rng.uniform(-1, 1), 3))
        if scheme == "central":
            for f in range(6):
                if types[f] in ("neumann", "symmetry"):
                    types[f], vals[f] = "dirichlet", round(rng.uniform(-1, 1), 3)
        if scheme == "quick" and types[0] == "periodic":
            types[0:2], vals[0:2] = ["dirichlet", "neumann"], [0.25, -0.5]
        form = rng.choice(["pos", "neg", "field", "self"])
        if scheme == "compat" and form == "neg":
            form = "field"
        stage = rng.choice([None, R.ALL4[rng.randrange(4)]])
        cap = rng.choice([k for k in (1, 2, 3, 4) if n0 // k >= 2])
        rows = rng.choice([0, 4])
        out.append({"n": [n0, n1, n2], "dtype": dtype, "bcs": (vals, types), "scheme": scheme, "form": form, "stage": stage,
                    "cap": cap, "rows": rows, "seed": rng.randrange(1 << 30)})
    return out


def run_sweep_case(p, before_tiled=None):
    """None, or what differs between the tiled launch and the generic one"""
    c = Case(p["n"], p["dtype"], p["bcs"], p["seed"])
    c.generic()
    gen = c.launch(p["scheme"], p["form"], p["stage"])
    if before_tiled is not None:
        before_tiled()
    c.tiled(p["cap"], p["rows"])
    out = c.launch(p["scheme"], p["form"], p["stage"])
    if not bool(torch.isfinite(gen).all()) or not bit_equal(out, gen):
        return where(out, gen)
    return None


def test_seeded_sweep():
    bad = []
    for p in sweep_cases(160):
        r = run_sweep_case(p)
        if r is not None:
            bad.append((p, r))
    assert not bad, told(bad, 4)


# ---- (e) the rule itself, no switch set: thin meshes that reach long chunks and four rows on a 256-CU part ----------------
def rule_child():
    res = {}

    def thin(n, dtype, bcs):
        c = Case(n, dtype, bcs, seed=3)
        assert c.ctx.get_option("chunks") == 0 and c.ctx.get_option("sf") == 1 and c.ctx.get_option("sfq") == 1
        return c

    # [256, 1010, 8] fp32, upwind NEUSYM, a 3-step march: 64 tiles of 16 rows, chunks of ~32 planes, four rows, BC on load
    c = thin([256, 1010, 8], "single", R.NEUSYM)
    _mark("march")
    out = _march(c, "upwind", False, 0, 1.3)
    _mark("-")
    c.generic()
    gen = _march(c, "upwind", False, 0, 1.3)
    res["march"] = (bit_equal(out, gen), meets("upwind", "single", out, _cpu_march(c, "upwind", False, 0, 1.3)))
    # the same shape fp64, central ALLDIR, one stage
    c = thin([256, 1010, 8], "double", R.ALLDIR)
    _mark("central")
    out = c.launch("central", "pos", R.ALL4[0])
    _mark("-")
    ref = c.cpu("central", "pos", R.ALL4[0])
    c.generic()
    res["central"] = (bit_equal(out, c.launch("central", "pos", R.ALL4[0])), meets("central", "double", out, ref))
    # [100, 509, 8]: QUICK (fp64, a speed field, one stage) and k_cg3d phase 3 through "sf" 0 (fp32, upwind step)
    c = thin([100, 509, 8], "double", R.MIXED)
    _mark("quick")
    out = c.launch("quick", "field", R.ALL4[1])
    _mark("-")
    ref = c.cpu("quick", "field", R.ALL4[1])
    c.generic()
    res["quick"] = (bit_equal(out, c.launch("quick", "field", R.ALL4[1])), meets("quick", "double", out, ref))
    c = thin([100, 509, 8], "single", R.MIXED)
    c.options(sf=0)
    _mark("cg3d")
    out = c.launch("upwind", "neg", None)
    _mark("-")
    ref = c.cpu("upwind", "neg", None)
    c.generic()
    res["cg3d"] = (bit_equal(out, c.launch("upwind", "neg", None)), meets("upwind", "single", out, ref))
    sys.stderr.write("RESULT %r\n" % (res,))
    assert all(v[0] and v[1][0] for v in res.values()), res


def test_the_rule_itself_reaches_long_chunks():
    log = G.child("import torch\nimport test_gpu_chunks as T\nT.rule_child()\n", drop_options=True)
    seen = _by_case(log)
    print([ln for ln in log.splitlines() if "[pyapes_hip] k_" in ln or ln.startswith("RESULT")])
    march = [ln for ln in seen["march"] if "k_sf " in ln]
    assert len(march) == 3 and all("(BC on load)" in ln and _field_of(ln, " RJ ") == 4 and _field_of(ln, "(CI ~") >= 5 for ln in march), seen["march"]
    cen = [ln for ln in seen["central"] if "k_sf " in ln]
    assert len(cen) == 1 and "(RK stage)" in cen[0] and _field_of(cen[0], " RJ ") == 4 and _field_of(cen[0], "(CI ~") >= 5, seen["central"]
    qk = [ln for ln in seen["quick"] if "k_sfq " in ln]
    assert len(qk) == 1 and "(RK stage)" in qk[0] and _field_of(qk[0], "(CI ~") >= 5, seen["quick"]
    cg = [ln for ln in seen["cg3d"] if "k_cg3d phase D" in ln]
    assert len(cg) == 1 and _field_of(cg[0], "(CI ~") >= 5 and not any("k_sf " in ln for ln in seen["cg3d"]), seen["cg3d"]


# ---- (f) CG and BiCGSTAB: the cap regroups the partial sums only ----------------------------------------------------------
def _fuzz_cases(seed, count, offset):
    """the first `count` 3-D cases of test_gpu_fuzz's seeded sequence that its own filters keep"""
    rng = random.Random(seed)
    out = []
    for case in range(2000):
        n, bcs, dtype = F._random_case(rng)
        if len(n) != 3 or (any(t == "periodic" for t, _ in bcs) and min(n) < 5) or not any(t == "dirichlet" for t, _ in bcs):
            continue
        tdt = torch.float64 if dtype == "double" else torch.float32
        g = torch.Generator().manual_seed(offset + case)
        rhs = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        x0 = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
        out.append((case, n, bcs, dtype, rhs, x0))
        if len(out) == count:
            break
    return out


def _oracle(n, bcs, dtype, rhs, x0, method, max_it):
    om = O.OMesh([0.0] * 3, [1.0 + 0.1 * a for a in range(3)], list(n), dtype)
    ocfg = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v} for i, (t, v) in enumerate(bcs)]
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            xo, ro = O.solve_poisson(om, ocfg, rhs.clone(), x0=x0.clone(), method=method, tol=-1.0, max_it=max_it, coeff=0.8, sign=-1.0)
    except RuntimeError:
        return None
    return (xo, ro) if bool(torch.isfinite(xo).all()) else None


def test_cg_under_a_cap(monkeypatch):
    """test_gpu_fuzz's product-versus-oracle comparison on 40 of its seeded 3-D cases, launch-per-phase loops ("resident" 0),
    caps 1 and 2: its tolerances, its iteration-count equality"""
    bad, ran = [], 0
    for case, n, bcs, dtype, rhs, x0 in _fuzz_cases(20261004, 40, 0):
        o = _oracle(n, bcs, dtype, rhs, x0, "cg", 2)
        if o is None:
            continue
        xo, ro = o
        hip_options(monkeypatch, resident=0, chunks=0)
        xg, rg, _ = F._product(n, bcs, dtype, rhs, x0, 3, False, monkeypatch)
        tol = 1e-10 if dtype == "double" else 2e-5
        for cap in (1, 2):
            hip_options(monkeypatch, resident=0, chunks=cap)
            xf, rf, _ = F._product(n, bcs, dtype, rhs, x0, 3, True, monkeypatch)
            ok = (rf["itr"] == rg["itr"] == ro["itr"] and rel_err(xf, xo) <= tol and rel_err(xg, xo) <= tol
                  and rel_err(xf, xg) <= (1e-12 if dtype == "double" else 1e-5))
            ran += 1
            if not ok:
                bad.append((case, n, [t for t, _ in bcs], dtype, cap, rel_err(xf, xo), rel_err(xg, xo), rel_err(xf, xg)))
    hip_options(monkeypatch, resident=None, chunks=None)
    assert ran >= 60, ran
    assert not bad, told(bad, 6)


def test_bicgstab_under_a_cap(monkeypatch):
    """the same for test_seeded_fuzz_bicgstab's comparison (three iterations), 24 of its 3-D cases"""
    bad, ran = [], 0

    def run(n, bcs, dtype, rhs, x0, fast):
        monkeypatch.setenv("PYAPES_HIP_FASTPATH", "1" if fast else "0")
        mesh = Mesh(Box([0.0] * 3, [1.0 + 0.1 * a for a in range(3)]), None, list(n), "cuda", dtype)
        cfg = [{"bc_face": O.FACES[i], "bc_type": t, "bc_val": v, "bc_val_opt": None} for i, (t, v) in enumerate(bcs)]
        var = Field("p", 1, mesh, {"domain": cfg, "obstacle": None})
        var.set_var_tensor(x0.cuda().clone())
        s = Solver({"fdm": {"method": "bicgstab", "tol": -1.0, "max_it": 3, "report": False}})
        s.set_eq(-FDM().laplacian(0.8, var) == rhs.cuda().clone())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rep = s.solve()
        return var().cpu(), rep

    for case, n, bcs, dtype, rhs, x0 in _fuzz_cases(20261005, 24, 1000):
        o = _oracle(n, bcs, dtype, rhs, x0, "bicgstab", 3)
        if o is None:
            continue
        xo, ro = o
        hip_options(monkeypatch, resident=0, chunks=0)
        xg, rg = run(n, bcs, dtype, rhs, x0, False)
        tol = 1e-9 if dtype == "double" else 5e-5
        for cap in (1, 2):
            hip_options(monkeypatch, resident=0, chunks=cap)
            xf, rf = run(n, bcs, dtype, rhs, x0, True)
            ok = (rf["itr"] == rg["itr"] == ro["itr"] and rel_err(xf, xo) <= tol and rel_err(xg, xo) <= tol
                  and rel_err(xf, xg) <= (1e-10 if dtype == "double" else 5e-5))
            ran += 1
            if not ok:
                bad.append((case, n, [t for t, _ in bcs], dtype, cap, rel_err(xf, xo), rel_err(xg, xo), rel_err(xf, xg), rf["itr"], rg["itr"], ro["itr"]))
    hip_options(monkeypatch, resident=None, chunks=None)
    monkeypatch.delenv("PYAPES_HIP_FASTPATH", raising=False)
    assert ran >= 30, ran
    assert not bad, told(bad, 6)
