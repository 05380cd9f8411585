"""The replay harness of tests/reuse_ops.py on fake operations (no GPU): a fake mesh whose "context" keeps a call counter,
options, the tensors its Python side holds for the library (``_keep``) and the raw pointers the "library" kept.  The harness
must report a planted history dependence at the step that has it, turn a planted read through a stale pointer into NaN and
report it, pass a clean catalogue, and refuse a comparison that left a step out -- so that tests/test_gpu_ctx_reuse.py
cannot pass vacuously."""
import pytest
import torch

import reuse_ops as RO
from reuse_ops import Carried, Op


class FakeCtx:
    def __init__(self):
        self.calls = 0          # what a context remembers: how often it was used (the sweep direction of the real one)
        self.options = {}
        self._keep = {}         # tensors held on behalf of the library
        self.raw_x = None       # "raw pointers" the library kept: the operand of the last binding ...
        self.raw_bc = None      # ... and its face values


class FakeMesh:
    def __init__(self):
        self._hip = FakeCtx()


def configure(mesh, options):
    mesh._hip.options.update(options)


def _input(seed):
    return torch.randn(16, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def clean_op(name, seed):
    """binds its own operand, every time"""
    def fn(mesh, carried):
        ctx = mesh._hip
        ctx.calls += 1
        x = _input(seed)
        carried.own(x)
        ctx.raw_x = x
        return {"y": ctx.raw_x * 2.0 + ctx.options.get("gain", 0), "n": int(x.numel()), "norm": float(x.norm())}
    return Op(name, fn, pure=True)


def option_op(value):
    def fn(mesh, carried):
        mesh._hip.options["gain"] = value
        carried.options["gain"] = value
        return {"gain": value}
    return Op(f"gain={value}", fn)


def carried_op():
    """reads and updates a carried field"""
    def fn(mesh, carried):
        mesh._hip.calls += 1
        acc = carried.fields.get("acc", torch.zeros(16, dtype=torch.float64)) + _input(3)
        carried.fields["acc"] = acc
        return {"acc": acc.clone()}
    return Op("accumulate", fn)


def history_op():
    """PLANTED: the sign of the last entry depends on how often the context was used before (an unreset toggle)"""
    def fn(mesh, carried):
        ctx = mesh._hip
        x = _input(5)
        y = x.clone()
        if ctx.calls % 2:
            y[-1] = -y[-1]
        ctx.calls += 1
        return {"y": y}
    return Op("history", fn)


def stale_pointer_op():
    """PLANTED: binds its operand only when nothing is bound yet -- else it reads through the pointer of an earlier binding
    (which held the SAME values: without poisoning the result would be right)"""
    def fn(mesh, carried):
        ctx = mesh._hip
        ctx.calls += 1
        x = _input(1)
        carried.own(x)
        if ctx.raw_x is None:
            ctx.raw_x = x
        return {"y": ctx.raw_x * 2.0}
    return Op("stale", fn)


def bind_bc_op(seed):
    def fn(mesh, carried):
        ctx = mesh._hip
        arr = _input(seed)
        ctx._keep["bc"] = [arr]      # an array the Python side made and holds: the caller never sees it
        ctx.raw_bc = arr
        return {"y": ctx.raw_bc + 1.0}
    return Op(f"bind_bc{seed}", fn, pure=True)


def lazy_rebind_op(seed):
    """PLANTED: the Python side swaps the held array, the "library" is never told and reads the dropped one"""
    def fn(mesh, carried):
        ctx = mesh._hip
        arr = _input(seed)
        ctx._keep["bc"] = [arr]
        if ctx.raw_bc is None:
            ctx.raw_bc = arr
        return {"y": ctx.raw_bc + 1.0}
    return Op(f"lazy_bc{seed}", fn, pure=True)


def test_a_clean_catalogue_passes():
    ops = [clean_op("a", 1), option_op(3), clean_op("b", 2), carried_op(), clean_op("a", 1), bind_bc_op(4), carried_op(),
           option_op(0), clean_op("a", 1), bind_bc_op(4)]
    steps = RO.check_script(ops, FakeMesh, configure)
    assert len(steps) == len(ops)
    assert torch.equal(steps[6].out["acc"], 2 * _input(3))         # the carried field really travelled
    assert float(steps[4].out["y"][0]) == float(_input(1)[0] * 2.0 + 3)     # ... and so did the option


def test_a_history_dependence_is_reported_at_its_step():
    ops = [clean_op("a", 1), history_op(), history_op(), clean_op("b", 2)]
    with pytest.raises(AssertionError) as e:
        RO.check_script(ops, FakeMesh, configure)
    msg = str(e.value)
    assert "step 1 (history) differs from its fresh run" in msg and "1 of 16 entries differ" in msg
    assert "step 2 (history)" not in msg and "step 0" not in msg and "step 3" not in msg      # (two uses before step 2: even again)
    RO.check_script([history_op(), clean_op("a", 1)], FakeMesh, configure)    # the first use of a context is a fresh one


def test_a_stale_pointer_read_turns_into_nan_and_is_reported():
    ops = [clean_op("a", 1), stale_pointer_op()]
    RO.check_script(ops, FakeMesh, configure, poisoning=False)     # same values behind the old pointer: invisible without
    with pytest.raises(AssertionError) as e:
        RO.check_script(ops, FakeMesh, configure)
    assert "step 1 (stale) differs from its fresh run" in str(e.value) and "(16 NaN here, 0 in the fresh run)" in str(e.value)
    steps = RO.run_script(ops, FakeMesh)
    assert bool(torch.isnan(steps[1].out["y"]).all()) and not bool(torch.isnan(steps[0].out["y"]).any())


def test_an_array_the_context_dropped_is_poisoned_too():
    ops = [bind_bc_op(4), lazy_rebind_op(4)]
    RO.check_script(ops, FakeMesh, configure, poisoning=False)
    steps = RO.run_script(ops, FakeMesh)
    assert not bool(torch.isnan(steps[1].out["y"]).any())      # dropped DURING step 1: poisoned after it ...
    ops.append(lazy_rebind_op(4))
    with pytest.raises(AssertionError, match=r"step 2 \(lazy_bc4\) differs from its fresh run"):     # ... and read by step 2
        RO.check_script(ops, FakeMesh, configure)


def test_the_step_count_condition_fires_when_a_step_is_dropped():
    ops = [clean_op("a", 1), clean_op("b", 2), clean_op("c", 3)]
    steps = RO.run_script(ops, FakeMesh)
    fresh = {s.k: RO.run_fresh(s.op, s.before, FakeMesh, configure) for s in steps}
    RO.verify(steps, fresh, len(ops))
    del fresh[1]
    with pytest.raises(AssertionError, match="2 steps compared, the script has 3"):
        RO.verify(steps, fresh, len(ops))
    with pytest.raises(AssertionError, match="steps compared"):
        RO.verify(steps[:2], {0: steps[0].out, 1: steps[1].out}, len(ops))      # a step that never ran


def test_a_repeated_pure_operation_must_equal_its_first_occurrence():
    """the fresh runs alone would not see two occurrences that BOTH equal their fresh run's twin in a script-only way: the
    repeats are compared with each other as well"""
    ops = [clean_op("a", 1), clean_op("b", 2), clean_op("a", 1)]
    steps = RO.run_script(ops, FakeMesh)
    fresh = {s.k: s.out for s in steps}
    RO.verify(steps, fresh, 3)
    steps[2].out["y"] = steps[2].out["y"] + 1.0
    fresh[2] = steps[2].out
    with pytest.raises(AssertionError, match=r"step 2 \(a\) differs from its first occurrence, step 0"):
        RO.verify(steps, fresh, 3)


def test_differences_are_exact():
    a = {"x": torch.tensor([1.0, float("nan")]), "itr": 3, "tol": 0.1, "s": {"alpha": float("nan")}}
    b = {"x": torch.tensor([1.0, float("nan")]), "itr": 3, "tol": 0.1, "s": {"alpha": float("nan")}}
    assert RO.differences(a, b) == []
    assert RO.differences(a, dict(b, tol=0.1 + 1e-18)) == []      # (the same float)
    assert len(RO.differences(a, dict(b, tol=0.1 * (1 + 3e-16)))) == 1
    assert len(RO.differences(a, dict(b, itr=4))) == 1
    assert len(RO.differences(a, dict(b, x=torch.tensor([1.0, 2.0])))) == 1
    assert len(RO.differences(a, {k: v for k, v in b.items() if k != "itr"})) == 1
    assert len(RO.differences(a, dict(b, x=torch.tensor([1.0, float("nan")], dtype=torch.float64)))) == 1


def test_snapshots_do_not_alias():
    c = Carried({"f": torch.ones(3)}, {"o": 1})
    s = c.snapshot()
    c.fields["f"].fill_(5.0)
    c.options["o"] = 2
    assert float(s.fields["f"][0]) == 1.0 and s.options == {"o": 1}
