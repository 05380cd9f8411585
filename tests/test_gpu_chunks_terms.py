"""-m gpu: the SOURCE (SRC) and VELOCITY (VEL) instantiations of the marching kernels over the meshes of tests/test_gpu_chunks.py.

tests/test_gpu_source.py and tests/test_gpu_velocity.py hold those instantiations against their CPU references on rows of 128 /
132 / 260 nodes, n1 = 13 / 14 / 16 and dirichlet / mixed faces.  k_sf takes its template parameters as `if constexpr` branches
inside one plane loop with rotating register slots, so an instantiation is tested there only on the shapes it has run on.  This
file runs them on the shapes of test_gpu_chunks.py -- chunks longer than one plane and every remainder of the chunk length mod 4,
one chunk with both axis-0 faces, one / two / four rows per wave and partial row blocks, rows of 32 .. 264 nodes, the eight BC
sets (a periodic axis 1 and 2 and all-Neumann / Neumann-symmetry faces among them) -- and on the edges that table lacks for the
two-row VEL kernels: n1 = 8 / 9 / 16 / 17 (exactly one row tile, a tile with one row) and the shortest row the vector kernels
take, 2 * VEC nodes, where one lane's vector ends the row.

Two yardsticks, neither of them the code under test, and no tolerance anywhere:
  * every tiled launch equals the generic kernels (option "fastpath" 0, "chunks" 0) in every bit;
  * the generic result, once per case, equals the CPU reference in every bit: tests/march_ref.py with one speed and
    with a velocity (tests/test_velocity_host.py holds the two forms against each other on these meshes).
Inputs: the case's two BC-filled fields and speed field, a source field 3 * randn and a velocity of three DISTINCT randn
components (a swapped axis cannot pass) from the case's seeded generator; the scalar velocity (0.9, -0.8, 0.4), the scalar
source 1.75.
"""
import random
import sys

import pytest
import torch

import march_gpu as G
import march_ref as M
import test_gpu_rk as R
from helpers import bit_equal
from pyapes_amd.solver.march import euler_march, rk_march
from test_gpu_chunks import (CAPS, CONFIG, DTYPES, MARCH_BCS, STAGES, Case, _by_case, _field_of, _mark, _n2, march_meshes, step_meshes,
                             told, where)

pytestmark = pytest.mark.gpu

LIMITER = {"upwind": "upwind", "central": "none", "quick": "quick"}      # the limiter names of tests/march_ref.py
SCALAR_VELOCITY = (0.9, -0.8, 0.4)
SCALAR_SOURCE = 1.75
SOURCES = ["field", "scalar"]


def _vec(dtype):
    return 2 if dtype == "double" else 4


class TermCase(Case):
    """a Case with a source field and a velocity, drawn from the case's seeded generator behind the draws of its fields"""

    def __init__(self, n, dtype, bcs, seed=17):
        super().__init__(n, dtype, bcs, seed)
        g = torch.Generator().manual_seed(seed)
        for draw in (torch.rand, torch.rand, torch.randn):     # the draws of test_gpu_rk._setup: two fields, the speed field
            draw((1, *n), generator=g, dtype=torch.float64)
        tdt = self.phis.dtype
        self.src_c = (3.0 * torch.randn((1, *n), generator=g, dtype=torch.float64)).to(tdt)
        self.vel_c = torch.randn((3, *n), generator=g, dtype=torch.float64).to(tdt)
        self.src, self.vel = self.src_c.cuda(), self.vel_c.cuda()
        self.x, self.x0, self.uf_c = self.phis.cpu().clone(), self.phi0.cpu().clone(), self.ufield.cpu().clone()

    def source(self, which):
        """(the reference's source, the device's as Case.launch takes it)"""
        if which is None:
            return None, None
        return (self.src_c, self.src[0]) if which == "field" else (SCALAR_SOURCE, SCALAR_SOURCE)

    def velocity(self, form):
        """(the reference's velocity, the device's), None where `form` names one speed"""
        if form == "vel_scalar":
            return list(SCALAR_VELOCITY), list(SCALAR_VELOCITY)
        if form == "vel_field":
            return [self.vel_c[a] for a in range(3)], [self.vel[a] for a in range(3)]
        return None, None

    def speed_ref(self, form):
        return self.uf_c if form == "field" else (self.x if form == "self" else self.speed(form))

    def run(self, scheme, form, stage, source):
        return self.launch(scheme, "pos" if form.startswith("vel_") else form, stage, self.source(source)[1], self.velocity(form)[1])

    def cpu_term(self, scheme, form, stage, source):
        s = self.source(source)[0]
        v = self.velocity(form)[0]
        u = v if v is not None else self.speed_ref(form)
        if stage is None:
            return M.euler_step(self.x, u, self.nu, self.dt, self.om, self.ob, LIMITER[scheme], s)
        return M.rk_stage(self.x, self.x0, stage[0], stage[1], u, self.nu, self.dt, self.om, self.ob, LIMITER[scheme], s)


def sweep_terms(dtype, scheme, form, meshes, rows_list, source):
    """every mesh x stage x rows x cap: tiled == generic in every bit, generic == the CPU reference in every bit"""
    bad, launches = [], 0
    for n, bcs in meshes:
        c = TermCase(n, dtype, bcs)
        c.generic()
        gen = [c.run(scheme, form, st, source) for st in STAGES]
        for st, g in zip(STAGES, gen):
            assert bool(torch.isfinite(g).all())
            ref = c.cpu_term(scheme, form, st, source)
            if not bit_equal(g, ref):
                bad.append((c.tag, scheme, form, source, "generic vs CPU", st, where(g.cpu(), ref)))
        for rows in rows_list:
            if rows == 4 and scheme != "quick" and not form.startswith("vel_") and n[1] <= 8:
                continue                      # k_sf: the one- and two-row rules stand in front of the forced value
            for cap in CAPS:
                c.tiled(cap, rows)
                for st, g in zip(STAGES, gen):
                    out = c.run(scheme, form, st, source)
                    launches += 1
                    if not bit_equal(out, g):
                        bad.append((c.tag, scheme, form, source, "rows", rows, "cap", cap, "stage", st, where(out, g)))
    assert not bad, told(bad, 6)
    return launches


# ---- (a) step and stage of the SRC instantiations -----------------------------------------------------------------------------
SF_SRC = [("upwind", "pos"), ("upwind", "neg"), ("upwind", "field"), ("upwind", "self"), ("central", "pos"), ("central", "self")]


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme,form", SF_SRC, ids=lambda v: v)
def test_k_sf_source_step_and_stage(scheme, form, dtype, source):
    assert sweep_terms(dtype, scheme, form, step_meshes(dtype, scheme, "k_sf"), (2, 4), source) > 200


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["pos", "neg", "field", "self"])
def test_k_sfq_source_step_and_stage(form, dtype, source):
    assert sweep_terms(dtype, "quick", form, step_meshes(dtype, "quick", "k_sfq"), (2, 4), source) > 200


# ---- (b) step and stage of the VEL instantiations -----------------------------------------------------------------------------
def vel_meshes(dtype):
    """the step meshes ([18, 4, 32] and the two meshes with a periodic axis 0 are declined: the generic kernel) and the row-count
    edges of the two-row kernels, TJ = 8: one full row tile, a tile with one row, two full tiles, two tiles and a row; the
    shortest row (2 * VEC nodes) at two rows of a partial tile and with a periodic axis 1"""
    short = 2 * _vec(dtype)
    return step_meshes(dtype, "upwind", "k_sf") + [([7, 8, 32], R.MIXED), ([7, 9, 32], R.ALLNEU), ([7, 16, 32], R.NEUSYM),
                                                   ([7, 17, _n2(34, dtype)], R.MIXED), ([7, 6, short], R.ALLDIR), ([7, 9, short], R.YPER)]


@pytest.mark.parametrize("source", [None] + SOURCES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["vel_scalar", "vel_field"])
def test_k_sf_velocity_step_and_stage(form, dtype, source):
    """option "sf" 2 and 4: a forced four runs the two-row kernel and gives the same bits"""
    assert sweep_terms(dtype, "upwind", form, vel_meshes(dtype), (2, 4), source) > 500


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_mix_of_scalar_and_field_components_under_a_cap(dtype):
    """pa_velocity with field[1] == NULL on [13, 19, a]: the vector kernel declines it whatever the options say, and the generic
    kernel gives the reference's bits"""
    c = TermCase([13, 19, _n2(34, dtype)], dtype, R.MIXED)
    v_ref, v_dev = [c.vel_c[0], -0.8, c.vel_c[2]], [c.vel[0], -0.8, c.vel[2]]
    ran = 0
    for source in (None, "field"):
        s_ref, s_dev = c.source(source)
        for st in STAGES:
            if st is None:
                ref = M.euler_step(c.x, v_ref, c.nu, c.dt, c.om, c.ob, "upwind", s_ref)
            else:
                ref = M.rk_stage(c.x, c.x0, st[0], st[1], v_ref, c.nu, c.dt, c.om, c.ob, "upwind", s_ref)
            c.generic()
            assert bit_equal(c.launch("upwind", "pos", st, s_dev, v_dev), ref), (source, st)
            for cap in (2, 0):
                for rows in (2, 4):
                    c.tiled(cap, rows)
                    out = c.launch("upwind", "pos", st, s_dev, v_dev)
                    ran += 1
                    assert bit_equal(out, ref), (source, st, cap, rows, where(out.cpu(), ref))
    assert ran == 24


# ---- (c) marches --------------------------------------------------------------------------------------------------------------
def _march(c, scheme, form, order, source):
    f = G.fresh_field(c.mesh, c.bc, c.phis)
    v = c.velocity(form)[1]
    u = tuple(v) if v is not None else (f if form == "self" else c.speed(form))
    s = c.src if source == "field" else c.source(source)[1]
    if order == 0:
        return euler_march(f, u, c.nu, c.dt, 3, CONFIG[scheme], source=s)().clone()
    return rk_march(f, u, c.nu, c.dt, 3, CONFIG[scheme], order=order, source=s)().clone()


def _cpu_march(c, scheme, form, order, source):
    s = c.source(source)[0]
    v = c.velocity(form)[0]
    if v is not None:
        return M.march(c.x, v, c.nu, c.dt, 3, c.om, c.ob, LIMITER[scheme], order or 1, s)
    return M.march(c.x, c.speed_ref(form), c.nu, c.dt, 3, c.om, c.ob, LIMITER[scheme], order or 1, s, self_adv=form == "self")


def sweep_term_marches(dtype, scheme, forms, orders, bcsets, source, bcl=(1,), extra=(), meshes=None, rows_list=(0, 4)):
    """three steps, caps 1 .. 3, the rule's rows and a forced four: tiled == generic == the CPU reference in every bit"""
    bad, launches = [], 0
    todo = [(n, bcs) for n in (meshes or march_meshes(dtype)) for bcs in bcsets] + list(extra)
    for n, bcs in todo:
        if scheme == "quick" and n[1] < 5:
            continue
        c = TermCase(n, dtype, bcs)
        for form in forms:
            for order in orders:   # 0: euler_march
                c.generic()
                gen = _march(c, scheme, form, order, source)
                assert bool(torch.isfinite(gen).all())
                ref = _cpu_march(c, scheme, form, order, source)
                if not bit_equal(gen, ref):
                    bad.append((c.tag, scheme, form, source, order, "generic vs CPU", where(gen.cpu(), ref)))
                for b in bcl:
                    for rows in rows_list:
                        if rows == 4 and scheme != "quick" and not form.startswith("vel_") and n[1] <= 8:
                            continue
                        for cap in (1, 2, 3):
                            c.tiled(cap, rows)
                            c.options(bcl=b)
                            out = _march(c, scheme, form, order, source)
                            launches += 1
                            if not bit_equal(out, gen):
                                bad.append((c.tag, scheme, form, source, "order", order, "bcl", b, "rows", rows, "cap", cap, where(out, gen)))
    assert not bad, told(bad, 6)
    return launches


def _yper(dtype):
    """a periodic face: the stage is the step plus k_rk_combine"""
    return [([7, 19, _n2(34, dtype)], R.YPER)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_euler_march_with_a_source(dtype):
    """euler_march, upwind, "bcl" 1 and 0: pa_sf_src_bcl.hip meets the rotating slots on 36, 20 and 6 rows"""
    assert sweep_term_marches(dtype, "upwind", ("pos", "neg", "field"), (0,), MARCH_BCS, "field", bcl=(1, 0)) > 400


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", ["upwind", "central", "quick"])
def test_rk_march_with_a_source(scheme, dtype):
    if scheme == "central":   # (central Div is refused on neumann / symmetry faces: ALLDIR alone, no YPER)
        assert sweep_term_marches(dtype, "central", ("pos",), (2, 3), [R.ALLDIR], "field") > 40
    else:
        assert sweep_term_marches(dtype, scheme, ("neg", "field"), (2, 3), MARCH_BCS, "field", extra=_yper(dtype)) > 300


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", ["upwind", "quick"])
def test_rk_march_self_advected_with_a_source(scheme, dtype):
    assert sweep_term_marches(dtype, scheme, ("self",), (3,), MARCH_BCS, "field", extra=_yper(dtype)) > 80


@pytest.mark.parametrize("source", [None, "field"], ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["vel_field", "vel_scalar"])
def test_marches_in_a_velocity(form, dtype, source):
    """euler_march and rk_march order 3, upwind, on the two-row VEL kernels"""
    assert sweep_term_marches(dtype, "upwind", (form,), (0, 3), MARCH_BCS, source, extra=_yper(dtype)) > 150


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scheme", ["quick", "central"])
def test_marches_in_a_velocity_on_the_generic_kernel(scheme, dtype):
    """no VEL instantiation of k_sfq or of central k_sf: pa_rk_march_vel's buffer rotation on the generic kernel, every order"""
    bcsets = [R.ALLDIR] if scheme == "central" else [R.MIXED]
    ran = 0
    for source in (None, "field"):
        ran += sweep_term_marches(dtype, scheme, ("vel_field", "vel_scalar"), (0, 2, 3), bcsets, source, meshes=[[13, 20, 36]], rows_list=(0,))
    assert ran == 36


# ---- (d) a seeded sweep -------------------------------------------------------------------------------------------------------
def _instantiation(p):
    """a key no finer than the kernel instantiation a case runs (the launch log prints eight lines per instantiation)"""
    form = p["form"]
    if p["scheme"] == "quick" and form == "self":
        form = "field"                               # k_sfq: SELF is the speed-field instantiation
    if p["scheme"] in ("central", "compat") and form in ("pos", "neg"):
        form = "scalar"                              # no sign of the speed in these instantiations
    fused = p["stage"] is not None and "periodic" not in p["bcs"][1]
    return (p["dtype"], p["scheme"], form, fused, p["source"] is not None)


def term_cases(count=160, seed=20261103):
    """cases the tiled kernels take BY CONSTRUCTION (the conditions of test_gpu_chunks.sweep_cases), drawn until `count` of them
    satisfy: a source not with the literal upwind form; central not with a foreign speed field; a velocity upwind only, without
    a periodic axis 0 (n1 >= 5 always); QUICK on rows of five nodes or more.  Reordered so that the first 24 -- whose launch
    lines test_term_sweep_cases_run_on_the_tiled_kernels reads -- stay within the log's budget per instantiation."""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        dtype = rng.choice(DTYPES)
        form = rng.choice(["pos", "neg", "field", "self", "vel_scalar", "vel_field"])
        scheme = "upwind" if form.startswith("vel_") else rng.choice(["upwind", "upwind", "compat", "central", "quick", "quick"])
        source = rng.choice([None, "scalar", "field"])
        n0, n1 = rng.randint(5, 23), rng.randint(5, 40)
        n2 = _n2(rng.choice([2 * _vec(dtype), 2 * _vec(dtype), 8, 12, 34, 64, 72, 132, 136, 260, 264]), dtype)
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
        stage = rng.choice([None, R.ALL4[rng.randrange(4)]])
        cap = rng.choice([k for k in (1, 2, 3, 4) if n0 // k >= 2])
        rows = rng.choice([0, 4])
        p = {"n": [n0, n1, n2], "dtype": dtype, "bcs": (vals, types), "scheme": scheme, "form": form, "stage": stage, "cap": cap,
             "rows": rows, "source": source, "seed": rng.randrange(1 << 30)}
        if scheme == "compat" and (source is not None or form == "neg"):
            continue
        if scheme == "central" and form == "field":
            continue
        if scheme == "quick" and (n2 < 5 or types[0] == "periodic"):
            continue
        if form.startswith("vel_") and types[0] == "periodic":
            continue
        out.append(p)
    first, rest, used = [], [], {}
    for p in out:
        k = _instantiation(p)
        if len(first) < 24 and used.get(k, 0) < 6:
            used[k] = used.get(k, 0) + 1
            first.append(p)
        else:
            rest.append(p)
    return first + rest


def run_term_case(p, before_tiled=None):
    """None, or what differs: generic vs the CPU reference (the literal upwind form has none), tiled vs generic"""
    c = TermCase(p["n"], p["dtype"], p["bcs"], p["seed"])
    c.generic()
    gen = c.run(p["scheme"], p["form"], p["stage"], p["source"])
    if not bool(torch.isfinite(gen).all()):
        return "not finite"
    if p["scheme"] in LIMITER:
        ref = c.cpu_term(p["scheme"], p["form"], p["stage"], p["source"])
        if not bit_equal(gen, ref):
            return ("generic vs CPU",) + where(gen.cpu(), ref)
    if before_tiled is not None:
        before_tiled()
    c.tiled(p["cap"], p["rows"])
    out = c.run(p["scheme"], p["form"], p["stage"], p["source"])
    if not bit_equal(out, gen):
        return ("tiled vs generic",) + where(out, gen)
    return None


def test_term_sweep_has_what_it_promises():
    ps = term_cases()
    assert len(ps) == 160
    assert sum(p["source"] is not None for p in ps) >= 40
    assert sum(p["form"].startswith("vel_") for p in ps) >= 40
    assert any(p["n"][2] == 2 * _vec(p["dtype"]) and p["form"].startswith("vel_") for p in ps)
    assert any(p["n"][2] == 2 * _vec(p["dtype"]) and p["source"] is not None for p in ps)
    for p in ps:
        vel, types = p["form"].startswith("vel_"), p["bcs"][1]
        assert not (p["source"] is not None and p["scheme"] == "compat")
        assert not (p["scheme"] == "central" and p["form"] == "field")
        assert not vel or (p["scheme"] == "upwind" and p["n"][1] >= 5 and types[0] != "periodic")
        assert p["n"][0] // p["cap"] >= 2
    used = {}
    for p in ps[:24]:
        used[_instantiation(p)] = used.get(_instantiation(p), 0) + 1
    assert max(used.values()) <= 8, used


def test_term_seeded_sweep():
    bad, ran = [], 0
    for p in term_cases():
        r = run_term_case(p)
        ran += 1
        if r is not None:
            bad.append((p, r))
    assert ran == 160, ran         # all of them, none skipped
    assert not bad, told(bad, 4)


def sweep_child():
    for k, p in enumerate(term_cases()[:24]):
        assert run_term_case(p, lambda: _mark("terms %d" % k)) is None, p
        _mark("-")
    torch.cuda.synchronize()


def test_term_sweep_cases_run_on_the_tiled_kernels():
    """the first 24 cases in one child process with the launch log on: one k_sf / k_sfq line each, with the source and the
    velocity it was given, the cap's chunks of two planes or more, and no generic or k_cg3d launch beside it"""
    log = G.child("import torch\nimport test_gpu_chunks_terms as T\nT.sweep_child()\n", drop_options=True)
    seen = _by_case(log)
    checked = 0
    for k, p in enumerate(term_cases()[:24]):
        assert "terms %d" % k in seen, (k, p, log[-2000:])
        mine = seen["terms %d" % k]
        lines = [ln for ln in mine if "k_sf " in ln or "k_sfq " in ln]
        assert len(lines) == 1, (p, mine)            # (no line at all is a failure: the case did not run where it should)
        ln = lines[0]
        assert ("k_sfq " in ln) == (p["scheme"] == "quick"), (p, ln)
        assert ("(source)" in ln) == (p["source"] is not None), (p, ln)
        assert ("(velocity)" in ln) == p["form"].startswith("vel_"), (p, ln)
        assert _field_of(ln, "chunks ") == p["cap"] and _field_of(ln, "(CI ~") >= 2, (p, ln)
        assert ("(RK stage)" in ln) == (p["stage"] is not None and "periodic" not in p["bcs"][1]), (p, ln)
        assert not any("k_euler" in x or "k_cg3d" in x for x in mine), (p, mine)
        checked += 1
    assert checked == 24


# ---- (e) the rule itself, no switch set ---------------------------------------------------------------------------------------
def rule_child():
    res = {}

    def thin(n, dtype, bcs):
        c = TermCase(n, dtype, bcs, seed=3)
        assert c.ctx.get_option("chunks") == 0 and c.ctx.get_option("sf") == 1 and c.ctx.get_option("sfq") == 1
        return c

    # [256, 1010, 8] fp32 NEUSYM, a 3-step upwind march with a source field: four rows by the rule, chunks of ~32 planes, BC on load
    c = thin([256, 1010, 8], "single", R.NEUSYM)
    _mark("march")
    out = _march(c, "upwind", "pos", 0, "field")
    _mark("-")
    c.generic()
    gen = _march(c, "upwind", "pos", 0, "field")
    res["march"] = (bit_equal(out, gen), bit_equal(gen, _cpu_march(c, "upwind", "pos", 0, "field")))
    # the same shape fp64 MIXED: one fused stage in a velocity of three fields with a scalar source, two rows
    c = thin([256, 1010, 8], "double", R.MIXED)
    _mark("velocity")
    out = c.run("upwind", "vel_field", R.ALL4[0], "scalar")
    _mark("-")
    c.generic()
    gen = c.run("upwind", "vel_field", R.ALL4[0], "scalar")
    res["velocity"] = (bit_equal(out, gen), bit_equal(gen, c.cpu_term("upwind", "vel_field", R.ALL4[0], "scalar")))
    sys.stderr.write("RESULT %r\n" % (res,))
    assert all(v[0] and v[1] for v in res.values()), res


def test_the_rule_itself_with_a_source_and_a_velocity():
    log = G.child("import torch\nimport test_gpu_chunks_terms as T\nT.rule_child()\n", drop_options=True)
    seen = _by_case(log)
    print([ln for ln in log.splitlines() if "[pyapes_hip] k_" in ln or ln.startswith("RESULT")])
    march = [ln for ln in seen["march"] if "k_sf " in ln]
    assert len(march) == 3 and all("(BC on load)" in ln and "(source)" in ln and _field_of(ln, " RJ ") == 4 and _field_of(ln, "(CI ~") >= 5
                                   for ln in march), seen["march"]
    vel = [ln for ln in seen["velocity"] if "k_sf " in ln]
    assert len(vel) == 1 and all(w in vel[0] for w in ("(velocity)", "(source)", "(RK stage)")), seen["velocity"]
    assert _field_of(vel[0], " RJ ") == 2 and _field_of(vel[0], "(CI ~") >= 5, vel
    assert not any("k_euler" in ln or "k_cg3d" in ln for ln in seen["march"] + seen["velocity"]), (seen["march"], seen["velocity"])
