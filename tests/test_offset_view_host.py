"""helpers.offset_view / guards_intact on CPU tensors: the misaligned operands of tests/test_gpu_unaligned.py and the
march tests are what they claim to be, and a store next to the array is seen."""
import pytest
import torch

from helpers import GUARD_SENTINEL, guards_intact, offset_view


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_offset_view_is_a_guarded_contiguous_view(dtype, k):
    t = torch.randn(3, 5, 7).to(dtype)
    view, alloc = offset_view(t, k)
    es = alloc.element_size()
    assert view.shape == t.shape and view.dtype == dtype and view.is_contiguous() and torch.equal(view, t)
    assert view.data_ptr() % 16 == (k * es) % 16
    front = (view.data_ptr() - alloc.data_ptr()) // es
    assert front >= 16 and alloc.numel() - front - t.numel() >= 16
    assert guards_intact(alloc, view)
    view.mul_(2.0)                       # a store inside the array: the allocation sees it, the guards do not
    assert torch.equal(alloc[front:front + t.numel()].view(t.shape), 2.0 * t) and guards_intact(alloc, view)
    for pos in (front - 1, front + t.numel(), 0, alloc.numel() - 1):
        keep = alloc[pos].clone()
        alloc[pos] = 0.0
        assert not guards_intact(alloc, view)
        alloc[pos] = keep
        assert guards_intact(alloc, view)
    alloc[front - 1] = -GUARD_SENTINEL   # bit for bit: not merely finite
    assert not guards_intact(alloc, view)


def test_offset_view_takes_a_larger_guard():
    view, alloc = offset_view(torch.zeros(10, dtype=torch.float32), 1, guard=40)
    front = (view.data_ptr() - alloc.data_ptr()) // 4
    assert front >= 40 and alloc.numel() - front - 10 >= 40 and view.data_ptr() % 16 == 4
