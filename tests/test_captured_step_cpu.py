"""CPU: the warm-up / capture / replay state machine of the captured steps (ratrack_amd/captured.py) against fakes -- the callbacks
are Python callables that log their calls, the tensors small CPU tensors."""
import pytest
import torch

from ratrack_amd.captured import CapturedStep, signature


class Fakes:
    """eager / capture / copy / replay that append to one log."""

    def __init__(self, fail_captures=0):
        self.log, self.fail = [], fail_captures

    def names(self):
        return [e[0] for e in self.log]

    def eager(self, args):
        self.log.append(("eager", args))
        return "eager-out"

    def capture(self, static):
        self.log.append(("capture", static))
        if self.fail:
            self.fail -= 1
            raise RuntimeError("capture failed")
        out = "out-%d" % self.names().count("capture")
        return out, lambda: self.log.append(("replay", out))

    def copy(self, pairs):
        self.log.append(("copy", pairs))

    def call(self, step, args, key=None):
        return step(signature(args) if key is None else key, args, self.eager, self.capture)


def make_args(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(2, 3, 5, generator=g), None, torch.randint(0, 9, (2, 4), generator=g, dtype=torch.int32)]


def storage(t):
    return t.untyped_storage().data_ptr()


def test_warmup_then_capture_then_replay():
    f = Fakes()
    step = CapturedStep(2, f.copy)
    assert (step.captured, step.ready, step.warmups) == (False, False, 0)
    for n in (1, 2):
        args = make_args(n)
        assert f.call(step, args) == "eager-out"
        assert f.log[-1][0] == "eager" and f.log[-1][1] is args, "a warm-up step runs on the caller's own list"
        assert (step.captured, step.ready, step.warmups) == (False, False, n)
    args = make_args(3)
    assert f.call(step, args) == "out-1"
    assert f.names() == ["eager", "eager", "capture", "copy", "replay"]
    static = f.log[2][1]
    assert len(static) == 3 and static[1] is None
    for s, a in ((static[0], args[0]), (static[2], args[2])):
        assert torch.equal(s, a) and s.dtype == a.dtype and s.is_contiguous() and storage(s) != storage(a)
    pairs = f.log[3][1]
    assert len(pairs) == 2 and all(len(p) == 2 for p in pairs)
    assert pairs[0][0] is static[0] and pairs[0][1] is args[0] and pairs[1][0] is static[2] and pairs[1][1] is args[2]
    assert (step.captured, step.ready, step.warmups) == (True, True, 2)

    # later steps replay: no second capture, the same static objects paired with the new arguments, one replay after the copy
    new = make_args(4)
    assert f.call(step, new) == "out-1"
    assert f.names() == ["eager", "eager", "capture", "copy", "replay", "copy", "replay"]
    pairs = f.log[5][1]
    assert len(pairs) == 2
    assert pairs[0][0] is static[0] and pairs[0][1] is new[0] and pairs[1][0] is static[2] and pairs[1][1] is new[2]
    assert step.captured and step.ready


def test_a_strided_argument_gets_a_contiguous_static_and_is_the_copy_source():
    f = Fakes()
    step = CapturedStep(0, f.copy)
    view = torch.arange(12.0).reshape(3, 4).t()
    assert not view.is_contiguous()
    f.call(step, [view])
    static = f.log[0][1][0]
    assert static.is_contiguous() and static.shape == view.shape and torch.equal(static, view) and storage(static) != storage(view)
    assert f.log[1][0] == "copy" and f.log[1][1][0][0] is static and f.log[1][1][0][1] is view


def test_a_new_key_warms_up_and_captures_again_and_so_does_the_old_key():
    f = Fakes()
    step = CapturedStep(1, f.copy)
    a, b = [torch.zeros(2, 3)], [torch.zeros(4, 3)]
    f.call(step, a), f.call(step, a)
    assert step.ready and f.names() == ["eager", "capture", "copy", "replay"]
    assert f.call(step, b) == "eager-out"
    assert (step.captured, step.ready, step.warmups) == (False, False, 1)
    assert f.call(step, b) == "out-2"
    assert step.ready and f.names()[4:] == ["eager", "capture", "copy", "replay"]
    assert f.log[6][1][0][0].shape == (4, 3)
    f.call(step, a)                      # a single slot: the first key's graph is gone
    assert not step.ready and step.warmups == 1
    assert f.call(step, a) == "out-3"
    assert f.names()[8:] == ["eager", "capture", "copy", "replay"] and f.names().count("capture") == 3
    # the key is the caller's: the same tensors under another key are another step
    f.call(step, a, key="other")
    assert not step.ready and f.names()[-1] == "eager"


def test_no_warmup_captures_on_the_first_call():
    f = Fakes()
    step = CapturedStep(0, f.copy)
    assert f.call(step, make_args(0)) == "out-1"
    assert f.names() == ["capture", "copy", "replay"] and step.captured and step.ready and step.warmups == 0


def test_a_failed_capture_leaves_no_graph_and_the_next_call_captures_again():
    f = Fakes(fail_captures=1)
    step = CapturedStep(1, f.copy)
    args = make_args(0)
    f.call(step, args)
    with pytest.raises(RuntimeError, match="capture failed"):
        f.call(step, args)
    assert f.names() == ["eager", "capture"]
    assert (step.captured, step.ready, step.warmups) == (False, False, 1)
    assert f.call(step, args) == "out-2"
    assert f.names() == ["eager", "capture", "capture", "copy", "replay"] and step.captured and step.ready
