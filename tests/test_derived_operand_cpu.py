"""derived.DerivedOperand: the key / rebuild / capture rule of weight-derived operands, driven with CPU tensors and a builder that records its calls.
torch.cuda.is_current_stream_capturing raises without a device, so every test that may reach it patches it; the hit-path test does not, on purpose."""
import copy

import pytest
import torch

from autosmoothquant_amd.derived import DerivedOperand, scale_vector


class Builder:
    """buffers = (2 * w, column sums) of the first input, written into `out` when given; records every call's `out`"""

    def __init__(self):
        self.outs = []

    def __call__(self, w, *rest, out=None):
        self.outs.append(out)
        if out is None:
            out = (torch.empty_like(w), torch.empty(w.shape[0], dtype=torch.int64))
        out[0].numpy()[...] = (w * 2).numpy()     # (raw writes: like the C-ABI, they bump no version counter the rule could see)
        out[1].numpy()[...] = w.sum(1).numpy()
        return out


def ptrs(buffers):
    return tuple(b.data_ptr() for b in buffers)


@pytest.fixture
def capturing(monkeypatch):
    state = {"on": False, "calls": 0}

    def fake():
        state["calls"] += 1
        return state["on"]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", fake)
    return state


def weight(seed=0, shape=(6, 8)):
    return torch.randint(-100, 100, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def test_hit_returns_the_same_buffers_without_any_other_torch_call(capturing, monkeypatch):
    op, build, w = DerivedOperand(), Builder(), weight()
    first = op.get((w,), build, w.shape)
    assert torch.equal(first[0], 2 * w) and build.outs == [None]
    capturing["on"] = True
    assert op.get((w,), build, w.shape) is first and build.outs == [None]      # a hit is a hit inside a capture too
    monkeypatch.undo()                                                          # is_current_stream_capturing is the real one again: it raises on this machine
    assert op.get((w,), build, w.shape) is first and build.outs == [None]
    assert capturing["calls"] == 1                                              # only the first (building) call asked


def test_miss_rebuilds_into_the_old_buffers_while_they_fit(capturing):
    op, build, w = DerivedOperand(), Builder(), weight()
    first = op.get((w,), build, w.shape)
    held = ptrs(first)
    w.add_(1)                                                                   # in place: the version counter moves, the storage stays
    got = op.get((w,), build, w.shape)
    assert build.outs[1] is first and len(build.outs) == 2 and ptrs(got) == held and torch.equal(got[0], 2 * w)
    w2 = weight(1)                                                              # a new tensor of the same shape
    got = op.get((w2,), build, w2.shape)
    assert build.outs[2] is first and len(build.outs) == 3 and ptrs(got) == held and torch.equal(got[0], 2 * w2)
    w3 = weight(2, (4, 8))                                                      # another declared shape: new buffers
    got = op.get((w3,), build, w3.shape)
    assert build.outs[3] is None and len(build.outs) == 4 and ptrs(got) != held and torch.equal(got[1], w3.sum(1))
    meta = torch.empty(4, 8, dtype=torch.int32, device="meta")                  # another device: the old buffers are not offered
    seen = []
    op.get((meta,), lambda w, out=None: seen.append(out) or (w, w), meta.shape)
    assert seen == [None]


def test_invalidate_gives_one_rebuild_in_place(capturing):
    op, build, w = DerivedOperand(), Builder(), weight()
    first = op.get((w,), build, w.shape)
    op.invalidate()
    assert ptrs(op.get((w,), build, w.shape)) == ptrs(first) and build.outs == [None, first]
    op.get((w,), build, w.shape)
    assert len(build.outs) == 2


def test_nothing_is_built_inside_a_capture(capturing):
    op, build, w = DerivedOperand(), Builder(), weight()
    capturing["on"] = True
    assert op.get((w,), build, w.shape) is None and build.outs == [] and op.buffers is None and op.key is None
    capturing["on"] = False
    first = op.get((w,), build, w.shape)
    assert first is not None and build.outs == [None]
    key, old = op.key, first[0].clone()
    w.add_(1)
    capturing["on"] = True
    assert op.get((w,), build, w.shape) is None                                 # a miss: no build, the cache as it was
    assert len(build.outs) == 1 and op.buffers is first and op.key == key and torch.equal(first[0], old)
    assert op.refresh((w,), build, w.shape) is False and len(build.outs) == 1   # refresh builds nothing either ...
    capturing["on"] = False
    got = op.get((w,), build, w.shape)                                          # ... and the next eager get rebuilds into the same buffers
    assert build.outs[1] is first and len(build.outs) == 2 and ptrs(got) == ptrs(first) and torch.equal(got[0], 2 * w)


def test_refresh_under_capture_leaves_the_operand_stale(capturing):
    """the sources are unchanged as far as torch can see (a raw write): only the stale mark makes the next eager get rebuild"""
    op, build, w = DerivedOperand(), Builder(), weight()
    first = op.get((w,), build, w.shape)
    capturing["on"] = True
    assert op.refresh((w,), build, w.shape) is False and len(build.outs) == 1
    capturing["on"] = False
    assert ptrs(op.get((w,), build, w.shape)) == ptrs(first) and build.outs == [None, first]
    assert DerivedOperand().refresh((w,), build, w.shape) is False and len(build.outs) == 2      # nothing held: nothing to refresh


def test_a_source_without_a_version_counter_needs_pin(capturing):
    op, build = DerivedOperand(), Builder()
    with torch.inference_mode():
        w = weight()
        with pytest.raises(RuntimeError):
            w._version
        assert op.get((w,), build, w.shape) is None and build.outs == [] and capturing["calls"] == 0
        op.pin()
        first = op.get((w,), build, w.shape)
        assert torch.equal(first[0], 2 * w) and build.outs == [None]
        w.add_(1)                                                               # not seen: the caller owns the refresh
        assert op.get((w,), build, w.shape) is first and len(build.outs) == 1 and not torch.equal(first[0], 2 * w)
        assert op.refresh((w,), build, w.shape) is True
        assert build.outs == [None, first] and ptrs(op.buffers) == ptrs(first) and torch.equal(op.buffers[0], 2 * w)


def test_out_of_memory_drops_the_operand_and_is_remembered(capturing):
    op, build, w = DerivedOperand(), Builder(), weight()

    def oom(w, out=None):
        raise torch.cuda.OutOfMemoryError("x")
    op.get((w,), build, w.shape)
    w.add_(1)
    assert op.get((w,), oom, w.shape) is None
    assert op.failed and op.buffers is None and op.key is None
    assert op.get((w,), build, w.shape) is not None and not op.failed and build.outs == [None, None]      # a later build that fits clears it

    def broken(w, out=None):
        raise ValueError("not an allocation failure")
    w.add_(1)
    with pytest.raises(ValueError):
        op.get((w,), broken, w.shape)
    assert not op.failed


def test_adopt_retires_the_former_buffers(capturing):
    op, build, w = DerivedOperand(), Builder(), weight()
    own = op.get((w,), build, w.shape)
    stack = (torch.zeros(12, 8, dtype=torch.int32), torch.zeros(12, dtype=torch.int64))
    mine = (stack[0][6:], stack[1][6:])
    got = op.adopt(mine, (w,), build, w.shape)
    assert got is mine and op.retired == [own] and build.outs == [None, mine]
    assert torch.equal(stack[0][6:], 2 * w) and torch.equal(stack[1][6:], w.sum(1)) and not stack[0][:6].any()
    w.add_(1)
    assert op.get((w,), build, w.shape) is mine and build.outs[2] is mine and torch.equal(stack[0][6:], 2 * w)
    assert op.adopt(mine, (w,), build, w.shape) is mine and op.retired == [own]                  # the same buffers again: nothing to retire
    wrong = (torch.zeros(5, 8, dtype=torch.int32), torch.zeros(5, dtype=torch.int64))
    assert op.adopt(wrong, (w,), build, w.shape) is None and op.buffers is mine                  # buffers that do not fit are refused


def test_an_operand_of_an_operand_is_keyed_on_the_original_sources(capturing):
    """the first operand is rebuilt in place by a builder that bumps no version counter; the second, which reads it, is rebuilt exactly once all the same"""
    first, second, b1, b2 = DerivedOperand(), DerivedOperand(), Builder(), Builder()
    g, u = weight(3), weight(4)

    def both():
        mid = first.get((g, u), b1, g.shape)
        return mid, second.get((g, u), b2, g.shape, inputs=(mid[0],))
    mid, img = both()
    assert torch.equal(img[0], 4 * g)
    both()
    assert len(b1.outs) == len(b2.outs) == 1
    ver = mid[0]._version
    g.add_(1)
    mid2, img2 = both()
    assert mid2[0]._version == ver and ptrs(mid2) == ptrs(mid) and ptrs(img2) == ptrs(img)
    assert len(b1.outs) == len(b2.outs) == 2 and b2.outs[1] is img and torch.equal(img2[0], 4 * g)
    both()
    assert len(b1.outs) == len(b2.outs) == 2


def test_a_deep_copy_rebuilds_for_itself(capturing):
    op, build, w = DerivedOperand(), Builder(), weight()
    first = op.get((w,), build, w.shape)
    snapshot = first[0].clone()
    twin = copy.deepcopy(op)
    w2 = weight(5)
    got = twin.get((w2,), build, w2.shape)
    assert ptrs(got) != ptrs(first) and torch.equal(got[0], 2 * w2) and torch.equal(first[0], snapshot)
    assert op.get((w,), build, w.shape) is first and len(build.outs) == 2


def test_scale_vector_is_rebuilt_when_a_value_moves_and_never_inside_a_capture():
    hit = scale_vector(None, (0.5, 2.0), (2, 3), "cpu")
    assert hit[1].tolist() == [0.5, 0.5, 2.0, 2.0, 2.0] and hit[1].dtype == torch.float32
    assert scale_vector(hit, (0.5, 2.0), (2, 3), "cpu", capturing=True) is hit
    assert scale_vector(hit, (0.5, 3.0), (2, 3), "cpu", capturing=True) is None
    assert scale_vector(hit, (0.5, 3.0), (2, 3), "cpu")[1].tolist() == [0.5, 0.5, 3.0, 3.0, 3.0]
