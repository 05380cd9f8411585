"""The edge-value fields of tests/edge_fields.py and the comparison ``helpers.same_bits``, checked on the CPU: the comparison
tells -0 from +0 and a subnormal from 0 and takes NaN as a class; every builder holds what it claims on every mesh that
tests/test_gpu_edge_values.py uses (the populations are printed); and the reference itself is determinate in bits on these
fields -- evaluated on the tensors as they are, on copies that start one element later inside a larger allocation, and with the
-0.0 cells of a speed replaced by +0.0 (torch.max(-0.0, 0.0) is +0 in the vectorised body of a tensor and -0 in its scalar
tail, so the sign of a zero speed half is no property of the reference).  The cells at which those evaluations differ are
AMBIGUOUS: they must be zeros, for the march forms there must be none (the accumulation (+0) + t_0 + t_1 + ... absorbs the
sign: the argument of DESIGN.md section 4 "Edge values", here checked on the reference), and for the general Div at most 1/16.
"""
import pytest
import torch

import edge_fields as E
from helpers import bit_equal, same_bits

MESHES = E.TILED + E.GENERIC
MESH_IDS = ["x".join(map(str, n)) + d[0] for n, d in MESHES]


def interior(t):
    return t[(0, *[slice(1, -1)] * (t.dim() - 1))]


# ---- same_bits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt,bits", [(torch.float32, torch.int32), (torch.float64, torch.int64)], ids=["f32", "f64"])
def test_same_bits(tdt, bits):
    t = torch.tensor([1.5, 0.0, -2.0, 3.0], dtype=tdt)
    assert same_bits(t, t.clone())
    neg = t.clone()
    neg[1] = -0.0
    assert bit_equal(t, neg) and not same_bits(t, neg)                       # -0 against +0
    r = same_bits(t, neg)
    assert "(1,)" in r.why and "0x8" in r.why and "0x0" in r.why, r.why      # the first index, both patterns
    sub = t.clone()
    sub[1] = torch.finfo(tdt).tiny / 16
    assert float(sub[1]) != 0.0 and not same_bits(t, sub)                    # a subnormal against 0
    quiet = torch.tensor([float("nan")], dtype=tdt)
    other = (quiet.view(bits) ^ torch.tensor([5], dtype=bits)).view(tdt)     # another payload
    minus = (-quiet)
    assert bool(torch.isnan(other).all()) and not torch.equal(quiet.view(bits), other.view(bits))
    assert not torch.equal(quiet.view(bits), minus.view(bits))
    a, b, c = t.clone(), t.clone(), t.clone()
    a[2], b[2], c[2] = quiet[0], other[0], minus[0]
    assert same_bits(a, b) and same_bits(a, c) and same_bits(b, c)           # NaNs of different sign and payload
    assert not same_bits(a, t) and not same_bits(t, a)                       # NaN against a number
    assert not same_bits(t, t.to(torch.float64 if tdt == torch.float32 else torch.float32))
    assert not same_bits(t, t[:3])
    inf = t.clone()
    inf[0] = float("inf")
    assert same_bits(inf, inf.clone()) and not same_bits(inf, -inf)


# ---- the builders hold what they claim ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dtype", MESHES, ids=MESH_IDS)
def test_zeros_field_population(n, dtype):
    f = E.zeros_field(n, dtype, 11)
    for name in ("phi", "phi0", "speed", "src"):
        x = interior(f[name])
        zeros, nonzero = int((x == 0).sum()), int((x != 0).sum())
        print("zeros_field %s %s %s: %d interior cells, %d zeros, %d non-zero" % (n, dtype, name, x.numel(), zeros, nonzero))
        assert 8 * zeros >= x.numel() and 8 * nonzero >= x.numel()
        whole = f[name][0]
        negz = (whole == 0) & torch.signbit(whole)
        assert int(negz.sum()) >= 1 and int(((whole == 0) & ~torch.signbit(whole)).sum()) >= 1
        assert negz.view(-1)[f["planted"][name]["negzero"]].all()
        if n[-1] >= 9:
            run = whole[E.block(n)]
            assert int(((run[..., 1:] == run[..., :-1]) & (run[..., 1:] != 0)).sum()) >= 1      # a flat run off zero
            assert int((run[..., 1:] * run[..., :-1] < 0).sum()) >= 1                           # a sign change
    for comp in f["vel"]:
        assert int(((comp == 0) & torch.signbit(comp)).sum()) >= 1 and int((comp > 0).sum()) >= 1 and int((comp < 0).sum()) >= 1
    half = n[0] // 2
    assert bool((f["nu"][:half] == 0).all()) and not bool(torch.signbit(f["nu"][:half]).any()) and bool((f["nu"][half:] > 0).all())


@pytest.mark.parametrize("n,dtype", MESHES, ids=MESH_IDS)
def test_positions_are_where_they_say(n, dtype):
    pos, v = E.positions(n, dtype), E.vec(dtype)
    for name, at in pos.items():
        assert len(at) == len(n) and all(0 <= i < m for i, m in zip(at, n)), (name, at)
        if name != "boundary":
            assert all(1 <= i <= m - 2 for i, m in zip(at, n)), (name, at)
    assert pos["boundary"][0] == 0 and pos["vector_last"][-1] % v == v - 1 and pos["vector_first"][-1] % v == 0
    assert v == 2 or pos["interior"][-1] % v not in (0, v - 1)      # (two lanes per vector: every cell is a first or a last one)
    if n[-1] > 64 * v + 2:
        assert pos["strip_last"][-1] == 64 * v - 1 and pos["strip_first"][-1] == 64 * v
    for a in range(len(n)):
        assert pos["axis%d_1" % a][a] == 1 and pos["axis%d_n2" % a][a] == n[a] - 2
    if len(n) == 3 and n[0] > 4:
        assert pos["chunk_first"][0] == pos["chunk_last"][0] + 1 == -(-n[0] // 2)
    t = torch.zeros((1, *n))
    for value in E.NONFINITE:
        p = E.planted(t, value, pos["interior"])
        assert int((~torch.isfinite(p)).sum()) == 1 and not bool(torch.isfinite(p[(0, *pos["interior"])])) and bool((t == 0).all())


def _classes(x, tdt):
    tiny = torch.finfo(tdt).tiny
    sub = (x != 0) & (x.abs() < tiny)
    normal = torch.isfinite(x) & (x.abs() >= tiny)
    return int(sub.sum()), int(normal.sum())


@pytest.mark.parametrize("n,dtype", MESHES, ids=MESH_IDS)
def test_reference_results_of_the_finite_classes(n, dtype):
    """subnormal: at least 1/8 of the interior cells of every result are non-zero subnormals and 1/8 normal; large: every
    result is finite; overflow: every result holds a NaN"""
    tdt = E.tdtype(dtype)
    low = [1.0, 1.0]
    for form in E.FINITE_FORMS:
        lim = E.FORMS[form][1]
        if lim in ("quick", "minmod", "mc") and min(n) < 5:
            continue
        bcname = "dir" if lim == "none" else "mix"
        for bc, stage in [(b, None) for b in E.form_bcs(form)] + [(bcname, E.STAGE)]:
            r = E.reference(E.case(n, dtype, bc, "subnormal"), form, stage)
            x = interior(r)
            sub, normal = _classes(x, tdt)
            low = [min(low[0], sub / x.numel()), min(low[1], normal / x.numel())]
            assert 8 * sub >= x.numel() and 8 * normal >= x.numel(), (form, bc, stage, sub, normal, x.numel())
        for stage in (None, E.STAGE):
            r = E.reference(E.case(n, dtype, bcname, "large"), form, stage)
            assert bool(torch.isfinite(r).all()), (form, stage)
            assert float(interior(r).abs().max()) > 1e-4 * torch.finfo(tdt).max * E.LARGE
            r = E.reference(E.case(n, dtype, bcname, "overflow"), form, stage)
            assert int(torch.isnan(r).sum()) >= 1, (form, stage)
    print("subnormal_field %s %s: smallest share of non-zero subnormal results %.3f, of normal results %.3f" % (n, dtype, *low))


# ---- how far the reference is determinate in bits -------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["zeros", "subnormal", "large"])
@pytest.mark.parametrize("n,dtype", MESHES, ids=MESH_IDS)
def test_march_forms_have_no_ambiguous_cell(n, dtype, cls):
    """euler_step and rk_stage of every form: the three evaluations agree in every bit"""
    total = 0
    for form in E.FINITE_FORMS:
        lim = E.FORMS[form][1]
        if lim in ("quick", "minmod", "mc") and min(n) < 5:
            continue
        c = E.case(n, dtype, "dir" if lim == "none" else "mix", cls)
        for stage in (None, E.STAGE):
            mask, ok = E.ambiguous(E.reference_variants(c, lambda **over: E.reference(c, form, stage, **over)))
            total += int(mask.sum())
            assert ok and int(mask.sum()) == 0, (form, stage, int(mask.sum()))
    print("AMBIGUOUS %s %s %s, march forms: %d cells" % (n, dtype, cls, total))


@pytest.mark.parametrize("cls", ["zeros", "subnormal", "large"])
@pytest.mark.parametrize("n,dtype", MESHES, ids=MESH_IDS)
def test_general_div_ambiguous_share(n, dtype, cls):
    """the literal upwind Div on the Ap / Ac / Am tables: at most 1/16 of the cells, all of them zeros"""
    for bcname in ("dir", "mix"):
        c = E.case(n, dtype, bcname, cls)
        mask, ok = E.ambiguous(E.reference_variants(c, lambda **over: E.general_div(c, **over)))
        print("AMBIGUOUS %s %s %s %s, general Div: %d of %d cells" % (n, dtype, cls, bcname, int(mask.sum()), mask.numel()))
        assert ok and 16 * int(mask.sum()) <= mask.numel()
