"""Deterministic fields made of the values that rand / randn never draw: exact zeros of both signs, flat runs, subnormals,
large magnitudes, two neighbours whose difference overflows, and single non-finite cells at the places where a tiled kernel changes hands.  A plain
module: no test lives here.  Every builder takes the mesh shape ``n``, the dtype ("single" / "double" or a torch dtype) and a
seed, and returns a dict of CPU tensors -- ``phi`` and ``phi0`` (1, *n), a ``speed`` (1, *n), a velocity ``vel`` (len(n), *n),
a diffusivity ``nu`` (*n), a source ``src`` (1, *n) -- and ``planted``: what it put where (flat indices into one component).
Nothing here knows about boundary conditions: a test fills the faces of ``phi`` / ``phi0`` itself.

    zeros_field      a compact block of random values and quarters on a background of exact +0, with flat runs (equal
                     neighbours along the last axis), exact zeros inside the block and -0.0 cells everywhere; speed, velocity
                     and source the same way (so: +0, -0 and sign changes between neighbours); nu exactly 0 on the lower half
                     of axis 0 (an insulating material) and positive on the upper half
    subnormal_field  k * tiny / 16 with integer |k| <= 64 -- subnormal below |k| = 16, normal up to 4 tiny -- and an O(1) cell
                     now and then; O(1) speeds and a positive nu with subnormal cells among them
    large_field      magnitudes of 2^-28 of the largest number: every operation of a step stays finite
    overflow_field   an O(1) field with two cells next to each other along the last axis at +-3/4 of the largest number: their
                     difference overflows
    positions        the named places of a mesh where a single cell is planted
    planted          a copy of a tensor with one cell replaced
"""
import contextlib

import torch

TDT = {"single": torch.float32, "double": torch.float64}
NONFINITE = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def tdtype(dtype):
    return dtype if isinstance(dtype, torch.dtype) else TDT[dtype]


def vec(dtype):
    """cells per 16-byte vector"""
    return 16 // torch.empty((), dtype=tdtype(dtype)).element_size()


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def block(n):
    """the compact block of a zeros_field: the middle 70 % of every axis"""
    return tuple(slice(-(-3 * m // 20), m - (-(-3 * m // 20))) for m in n)


def _mixed(n, g, tdt):
    """random values and the grid of quarters, cell by cell one or the other, with flat runs along the last axis"""
    r = torch.randn(tuple(n), generator=g, dtype=torch.float64)
    q = torch.randint(-8, 9, tuple(n), generator=g).to(torch.float64) / 4
    v = torch.where(torch.rand(tuple(n), generator=g, dtype=torch.float64) < 0.5, q, r).to(tdt)
    src = v[..., 2::5]
    dst = v[..., 3::5]
    dst.copy_(src[..., :dst.shape[-1]])          # cell 5 m + 3 repeats cell 5 m + 2
    return v


def _compact(n, g, tdt):
    """(the block on +0 with planted zeros, flat indices of the planted +0 cells, of the planted -0.0 cells)"""
    v = _mixed(n, g, tdt)
    out = torch.zeros(tuple(n), dtype=tdt)
    out[block(n)] = v[block(n)]
    flat = out.view(-1)
    zero = torch.arange(3, flat.numel(), 7)
    neg = torch.arange(5, flat.numel(), 11)
    flat[zero] = 0.0
    flat[neg] = -0.0
    return out, zero.tolist(), neg.tolist()


def zeros_field(n, dtype, seed):
    tdt, g, nd = tdtype(dtype), _gen(seed), len(n)
    out, planted = {}, {}
    for name in ("phi", "phi0", "speed", "src"):
        t, zero, neg = _compact(n, g, tdt)
        out[name] = t.unsqueeze(0)
        planted[name] = {"zero": zero, "negzero": neg}
    comps = [_compact(n, g, tdt) for _ in range(nd)]
    out["vel"] = torch.stack([c[0] for c in comps])
    planted["vel"] = [{"zero": c[1], "negzero": c[2]} for c in comps]
    nu = (1e-3 * (0.5 + torch.rand(tuple(n), generator=g, dtype=torch.float64))).to(tdt)
    nu[:n[0] // 2] = 0.0
    out["nu"] = nu
    planted["nu"] = {"zero_planes": n[0] // 2}
    out["planted"] = planted
    return out


def _subnormal(n, g, tdt, every):
    """k * tiny / 16, |k| <= 64, and an O(1) cell at every ``every``-th flat index; returns (tensor, those indices)"""
    unit = torch.tensor(torch.finfo(tdt).tiny / 16, dtype=tdt)
    assert float(unit) > 0.0 and float(unit) * 16 == torch.finfo(tdt).tiny
    k = torch.where(torch.rand(tuple(n), generator=g, dtype=torch.float64) < 0.7,
                    torch.randint(-15, 16, tuple(n), generator=g), torch.randint(-64, 65, tuple(n), generator=g)).to(tdt)
    t = k * unit                                   # exact: a multiple of a power of two inside the subnormal grid
    big = torch.randn(tuple(n), generator=g, dtype=torch.float64).to(tdt)
    idx = torch.arange(7, t.numel(), every)
    t.view(-1)[idx] = big.view(-1)[idx]
    return t, idx.tolist()


def _sprinkled(base, g, tdt, every, positive=False):
    """``base`` with a subnormal value at every ``every``-th flat index; returns (tensor, those indices)"""
    unit = torch.tensor(torch.finfo(tdt).tiny / 16, dtype=tdt)
    k = torch.randint(1, 16, tuple(base.shape), generator=g).to(tdt)
    if not positive:
        k = k * (2 * torch.randint(0, 2, tuple(base.shape), generator=g).to(tdt) - 1)
    idx = torch.arange(4, base.numel(), every)
    t = base.clone()
    t.view(-1)[idx] = (k * unit).view(-1)[idx]
    return t, idx.tolist()


def subnormal_field(n, dtype, seed):
    tdt, g, nd = tdtype(dtype), _gen(seed), len(n)
    out, planted = {}, {}
    for name in ("phi", "phi0", "src"):
        t, idx = _subnormal(n, g, tdt, 199)
        out[name] = t.unsqueeze(0)
        planted[name] = {"order_one": idx}
    comps = []
    for _ in range(nd + 1):
        base = torch.randn(tuple(n), generator=g, dtype=torch.float64).to(tdt)
        comps.append(_sprinkled(base, g, tdt, 9))
    out["speed"] = comps[0][0].unsqueeze(0)
    planted["speed"] = {"subnormal": comps[0][1]}
    out["vel"] = torch.stack([c[0] for c in comps[1:]])
    planted["vel"] = [{"subnormal": c[1]} for c in comps[1:]]
    nu = (1e-3 * (0.5 + torch.rand(tuple(n), generator=g, dtype=torch.float64))).to(tdt)
    out["nu"], idx = _sprinkled(nu, g, tdt, 13, positive=True)
    planted["nu"] = {"subnormal": idx}
    out["planted"] = planted
    return out


LARGE = 2.0 ** -28     # of the largest number: 1 / dx^2 <= 2^17 on the suite's meshes, a stencil sums < 2^5 such products


def large_field(n, dtype, seed):
    tdt, g, nd = tdtype(dtype), _gen(seed), len(n)
    scale = torch.finfo(tdt).max * LARGE

    def big(lead):
        return (torch.randn((lead, *n), generator=g, dtype=torch.float64) * scale).to(tdt)

    out = {"phi": big(1), "phi0": big(1), "src": big(1)}
    # a field that advects itself multiplies two of its values: 2^-14 of the square root of the largest number
    root = float(torch.finfo(tdt).max) ** 0.5 * 2.0 ** -14
    for name in ("self_phi", "self_phi0"):
        out[name] = (torch.randn((1, *n), generator=g, dtype=torch.float64) * root).to(tdt)
    out["speed"] = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
    out["vel"] = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(tdt)
    out["nu"] = (1e-3 * (0.5 + torch.rand(tuple(n), generator=g, dtype=torch.float64))).to(tdt)
    out["planted"] = {"scale": scale, "self_scale": root}
    return out


def plain_field(n, dtype, seed):
    """rand / randn fields, the background of the single planted cells"""
    tdt, g, nd = tdtype(dtype), _gen(seed), len(n)
    out = {name: torch.rand((1, *n), generator=g, dtype=torch.float64).to(tdt) for name in ("phi", "phi0")}
    out["src"] = (3.0 * torch.randn((1, *n), generator=g, dtype=torch.float64)).to(tdt)
    out["speed"] = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
    out["vel"] = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(tdt)
    out["nu"] = (1e-3 * (0.5 + torch.rand(tuple(n), generator=g, dtype=torch.float64))).to(tdt)
    out["planted"] = {}
    return out


def overflow_field(n, dtype, seed):
    """an O(1) case whose ``phi`` holds +3/4 max and -3/4 max at the interior position and its successor along the last axis"""
    tdt, g, nd = tdtype(dtype), _gen(seed), len(n)
    out = {name: torch.rand((1, *n), generator=g, dtype=torch.float64).to(tdt) for name in ("phi", "phi0")}
    out["src"] = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
    out["speed"] = torch.randn((1, *n), generator=g, dtype=torch.float64).to(tdt)
    out["vel"] = torch.randn((nd, *n), generator=g, dtype=torch.float64).to(tdt)
    out["nu"] = (1e-3 * (0.5 + torch.rand(tuple(n), generator=g, dtype=torch.float64))).to(tdt)
    at = positions(n, dtype)["interior"]
    nxt = at[:-1] + (at[-1] + 1,)
    big = 0.75 * torch.finfo(tdt).max
    out["phi"][(0, *at)] = big
    out["phi"][(0, *nxt)] = -big
    out["speed"][(0, *at)] = 0.5       # a positive speed at the first cell: its forward difference, -inf, meets u- = 0
    out["vel"][(slice(None), *at)] = 0.5
    out["planted"] = {"cells": [at, nxt]}
    return out


BUILDERS = {"plain": plain_field, "zeros": zeros_field, "subnormal": subnormal_field, "large": large_field, "overflow": overflow_field}


def positions(n, dtype, chunks=2):
    """{name: index} of the places where one cell is planted, as far as the mesh has them.  The last axis is the one the
    tiled kernels vectorise (16-byte vectors, a wave's strip is 64 of them), axis 1 the one they block by rows (2 or 4 per
    wave, counted from row 0: rows 3 | 4 are a border at both), axis 0 the one they march along in ``chunks`` chunks."""
    n = list(n)
    nd, v = len(n), vec(dtype)
    mid = [m // 2 for m in n]
    if mid[-1] % v == v - 1 or mid[-1] % v == 0:       # keep "interior" off the vector borders
        mid[-1] += 1 if mid[-1] + 2 < n[-1] - 1 else -1
    out = {"interior": tuple(mid)}

    def along(axis, i):
        p = list(mid)
        p[axis] = i
        return tuple(p)

    if n[-1] > 2 * v + 2:
        out["vector_last"], out["vector_first"] = along(nd - 1, 2 * v - 1), along(nd - 1, 2 * v)
    if n[-1] > 64 * v + 2:
        out["strip_last"], out["strip_first"] = along(nd - 1, 64 * v - 1), along(nd - 1, 64 * v)
    if nd >= 2 and n[-2] > 6:
        out["rows_last"], out["rows_first"] = along(nd - 2, 3), along(nd - 2, 4)
    if nd == 3:
        for tag, cut in (("", -(-n[0] // chunks)), ("_floor", n[0] // chunks)):
            if 1 < cut < n[0] - 1:
                out["chunk_last" + tag], out["chunk_first" + tag] = along(0, cut - 1), along(0, cut)
    for a in range(nd):
        out["axis%d_1" % a], out["axis%d_n2" % a] = along(a, 1), along(a, n[a] - 2)
    out["boundary"] = along(0, 0)
    return out


def distinct_positions(n, dtype, chunks=2):
    """[(names, index)] of ``positions``, every index once"""
    seen = {}
    for name, at in positions(n, dtype, chunks).items():
        seen.setdefault(at, []).append(name)
    return [("/".join(names), at) for at, names in seen.items()]


def planted(t, value, where, comp=0):
    """a copy of ``t`` -- one component's shape, or with a leading component axis -- holding ``value`` ("nan", "+inf", "-inf"
    or a number) at the mesh index ``where`` (of component ``comp``)"""
    t = t.clone()
    value = NONFINITE.get(value, value)
    if t.dim() == len(where):
        t[tuple(where)] = value
    else:
        assert t.dim() == len(where) + 1
        t[(comp, *where)] = value
    return t


def shifted(t, k=1):
    """``t`` as a contiguous view that starts ``k`` elements into a larger allocation: the same values on other vector lanes"""
    buf = torch.empty(t.numel() + k + 8, dtype=t.dtype)
    view = buf[k:k + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + k * t.element_size()
    return view


def without_negative_zero(t):
    """``t`` with every -0.0 replaced by +0.0: an equal VALUE everywhere"""
    return torch.where(t == 0, torch.zeros_like(t), t)


# ---- the cases the host and the GPU tests share: a mesh, a BC set and a class of fields ---------------------------------
TILED = [([14, 12, 16], "double"), ([10, 12, 132], "double"), ([6, 7, 260], "single"), ([9, 14, 260], "single")]
GENERIC = [([6, 7, 9], "double"), ([17, 12], "double"), ([33], "single")]
STAGE = (0.75, 0.25)
NU = 1e-3

# form: (kernel family on a tiled mesh, limiter of march_ref, speed -- a number, "field", "self" or "vel" --, source, nu field)
FORMS = {
    "sf_up_pos": ("k_sf", "upwind", 0.7, False, False),
    "sf_up_neg": ("k_sf", "upwind", -0.7, False, False),
    "sf_up_zero": ("k_sf", "upwind", 0.0, False, False),
    "sf_up_negzero": ("k_sf", "upwind", -0.0, False, False),
    "sf_up_field": ("k_sf", "upwind", "field", False, False),
    "sf_self_up": ("k_sf", "upwind", "self", False, False),
    "sf_self_cen": ("k_sf", "none", "self", False, False),
    "sf_vel": ("k_sf", "upwind", "vel", False, False),
    "sf_src": ("k_sf", "upwind", 0.7, True, False),
    "sf_src_field": ("k_sf", "upwind", "field", True, False),
    "sfn_u0": ("k_sfn", "upwind", 0.0, False, True),
    "sfn_neg": ("k_sfn", "upwind", -0.7, False, True),
}
for _lim in ("quick", "minmod", "mc"):
    for _tag, _u in (("pos", 0.7), ("neg", -0.7), ("field", "field"), ("self", "self")):
        FORMS["sfq_%s_%s" % (_lim, _tag)] = ("k_sfq", _lim, _u, False, False)


FINITE_FORMS = list(FORMS)
# a scalar speed of NaN: the library takes it like any other number, and the result is the reference's (NaN at every node
# of the interior set) on every kernel
FORMS["sf_up_nan"] = ("k_sf", "upwind", float("nan"), False, False)
FORMS["sfq_quick_nan"] = ("k_sfq", "quick", float("nan"), False, False)
FORMS["sfn_nan"] = ("k_sfn", "upwind", float("nan"), False, True)
NAN_SPEED_FORMS = [f for f in FORMS if f not in FINITE_FORMS]


def family_forms(family, forms=None):
    return [f for f in (FINITE_FORMS if forms is None else forms) if FORMS[f][0] == family]


def us_sign(form):
    """+1 / -1 where the tiled kernel of ``form`` takes the sign of a scalar speed as a launch-time fact and leaves the
    dead half of every axis term out (the US instantiations of k_sf / k_sfq: upwind, quick, minmod, mc), else 0"""
    fam, lim, u, src, nuf = FORMS[form]
    if fam not in ("k_sf", "k_sfq") or isinstance(u, str) or lim == "none":
        return 0
    return -1 if u < 0 else 1


def form_bcs(form):
    """the BC sets a form runs with (central Div refuses neumann / symmetry faces)"""
    return ("dir", "xper", "zper") if FORMS[form][1] == "none" else ("dir", "mix", "xper", "zper")


_CASES = {}


def case(n, dtype, bcname, cls, seed=11):
    """the oracle's mesh and BCs of the unit box with ``n`` nodes, the fields of class ``cls`` (a name of BUILDERS) with the
    faces of phi / phi0 filled (class "subnormal": the set's face values times tiny), the velocity as a list of components, ``nu_field`` beside the number ``nu``, and dt"""
    import pyapes_oracle as O
    from march_gpu import BCS, ZPER
    key = (tuple(n), dtype, bcname, cls, seed)
    if key not in _CASES:
        nd = len(n)
        vals, types = dict(BCS, zper=ZPER)[bcname]
        vals, types = vals[:2 * nd], types[:2 * nd]
        if cls == "subnormal":   # the face values belong to the class too: O(1) faces would leave few subnormal results
            tiny = float(torch.finfo(tdtype(dtype)).tiny)
            vals = [None if v is None else v * tiny for v in vals]
        om = O.OMesh([0.0] * nd, [1.0] * nd, list(n), dtype)
        obcs = O.make_bcs(om, O.mixed_cfg(vals, types, O.FACES[:2 * nd]))
        f = BUILDERS[cls](n, dtype, seed)
        for name in ("phi", "phi0", "self_phi", "self_phi0"):
            if name in f:
                O.bc_fill(f[name], obcs)
        dx = min(float(d) for d in om.dx)
        c = dict(n=list(n), dtype=dtype, bcname=bcname, cls=cls, om=om, obcs=obcs, vals=vals, types=types, nu=NU,
                 dt=0.2 * min(dx * dx / (2 * nd * NU), dx / 1.3), phi=f["phi"], phi0=f["phi0"], speed=f["speed"],
                 vel=[f["vel"][a].contiguous() for a in range(nd)], nu_field=f["nu"], src=f["src"], planted=f["planted"],
                 self_phi=f.get("self_phi"), self_phi0=f.get("self_phi0"))
        _CASES[key] = c
    return _CASES[key]


def operands(c, form, **over):
    """(phi, phi0, u, nu, S) of ``form`` on the case ``c`` as march_ref takes them; ``over``: replacements of phi, phi0,
    speed, vel, nu_field, src"""
    fam, lim, u, src, nuf = FORMS[form]
    own = u == "self" and c["self_phi"] is not None    # the class has fields of its own for self-advection

    def get(k):
        k = "self_" + k if own and k in ("phi", "phi0") else k
        return over.get(k, c[k])

    phi = get("phi")
    uu = {"field": get("speed"), "self": phi, "vel": list(get("vel"))}.get(u, u) if isinstance(u, str) else u
    return phi, get("phi0"), uu, (get("nu_field") if nuf else c["nu"]), (get("src") if src else None)


def reference(c, form, stage=None, e=None, **over):
    """march_ref's Euler step (``stage`` None) or stage of ``form``; ``e``: the stage's Euler value where it is known"""
    import march_ref as R
    phi, phi0, u, nu, S = operands(c, form, **over)
    lim = FORMS[form][1]
    if e is None:
        e = R.euler_step(phi, u, nu, c["dt"], c["om"], c["obcs"], lim, S)
    if stage is None:
        return e
    return R.rk_stage(phi, phi0, stage[0], stage[1], u, nu, c["dt"], c["om"], c["obcs"], lim, S, step=lambda *a: e)


def reference_variants(c, evaluate):
    """``evaluate(**over)`` on the case's tensors as they are, on copies that start one element into a larger allocation,
    with every -0.0 of a speed replaced by +0.0 (what max(u, 0) / min(u, 0) may make of it anyway), and without the two outer
    tables of the oracle's five-point sums (``three_point``)"""
    names = [k for k in ("phi", "phi0", "self_phi", "self_phi0", "speed", "nu_field", "src") if c[k] is not None]
    moved = {k: shifted(c[k]) for k in names}
    moved["vel"] = [shifted(t) for t in c["vel"]]
    plus = {"speed": without_negative_zero(c["speed"]), "vel": [without_negative_zero(t) for t in c["vel"]]}
    with three_point():
        inner = evaluate()
    return evaluate(), evaluate(**moved), evaluate(**plus), inner


def ambiguous(results):
    """(AMBIGUOUS, ok): the cells at which evaluations of the reference differ in bits, and whether every one of them is a
    zero in all evaluations"""
    from helpers import _BITS
    first = results[0]
    mask = torch.zeros(first.shape, dtype=torch.bool)
    for r in results[1:]:
        nan = torch.isnan(first) | torch.isnan(r)
        mask |= (torch.isnan(first) != torch.isnan(r)) | (~nan & (first.view(_BITS[first.dtype]) != r.view(_BITS[r.dtype])))
    ok = all(bool((r[mask] == 0).all()) for r in results)
    return mask, ok


def dead_half_nonfinite(c, form, phi):
    """the cells at which the half that a US kernel leaves out is not finite on some axis: fwd / fq for u >= 0, bwd / bq for
    u < 0 -- where the literal form has 0 * (inf or NaN) = NaN and the US kernel nothing"""
    import march_ref as R
    sign, lim = us_sign(form), FORMS[form][1]
    assert sign != 0
    x = phi[0]
    periodic = [False] * x.dim()
    for bc in c["obcs"]:
        if bc.type == "periodic":
            periodic[c["om"].axis_of(bc.face)] = True
    bad = torch.zeros(x.shape, dtype=torch.bool)
    for a in range(x.dim()):
        if lim == "upwind":
            bq, fq = x - torch.roll(x, 1, a), torch.roll(x, -1, a) - x
        elif lim == "quick":
            bq, fq = R.quick_halves(x, a, periodic[a])
        else:
            bq, fq, _, _ = R.tvd_halves(x, a, periodic[a], lim)
        bad |= ~torch.isfinite(fq if sign > 0 else bq)
    return bad.unsqueeze(0)


def general_div(c, **over):
    """the oracle's general Div in the literal upwind form (``compat``: the Ap / Ac / Am tables) of the case's phi with its
    speed field"""
    import pyapes_oracle as O
    phi, speed = over.get("phi", c["phi"]), over.get("speed", c["speed"])
    return O.apply_div(O.div_tables(speed, phi, c["om"], c["obcs"], "upwind"), phi, c["om"].dim)



@contextlib.contextmanager
def three_point():
    """While active the oracle's stencil sums leave out the two outer tables of its five-point form (its own switch,
    ``pyapes_oracle.SKIP_OUTER_TABLES``, which also asserts that they are zero).  On finite fields nothing changes, not even
    a bit (a sum that starts at +0 absorbs the +-0 they contribute); two nodes away from a non-finite cell they make 0 * (inf or NaN) = NaN where a kernel,
    which reads three points per axis, has a number."""
    import pyapes_oracle as O
    before = O.SKIP_OUTER_TABLES
    O.SKIP_OUTER_TABLES = True
    try:
        yield
    finally:
        O.SKIP_OUTER_TABLES = before


def through_bc_fill(mask, c):
    """``mask`` (1, *n) and the boundary nodes whose fill reads a cell of it: a marker field, NaN on the mask, through the
    oracle's BC fill"""
    import pyapes_oracle as O
    m = torch.where(mask, torch.full((), float("nan"), dtype=c["phi"].dtype), torch.zeros((), dtype=c["phi"].dtype))
    O.bc_fill(m, c["obcs"])
    return mask | torch.isnan(m)
