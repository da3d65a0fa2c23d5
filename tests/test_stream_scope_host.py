"""(no GPU) `main._on_torch_stream`: the cached handle goes back to its own stream whatever fails inside the scope or in its
drain.  The handle is a fake that records its calls; torch's device and stream calls are replaced, so nothing reaches a GPU."""
import contextlib
from types import SimpleNamespace

import pytest


class FakeHandle:
    def __init__(self, drain_error=None):
        self.calls, self.drain_error = [], drain_error

    def set_stream(self, stream):
        self.calls.append(("set_stream", stream))

    def synchronize(self):
        self.calls.append(("synchronize",))
        if self.drain_error is not None:
            raise self.drain_error


@pytest.fixture
def no_gpu(monkeypatch):
    """torch.cuda.device and torch.cuda.current_stream as recorders: (log of their calls)."""
    import torch
    log = []

    @contextlib.contextmanager
    def device(dev):
        log.append(("enter", str(dev)))
        yield
        log.append(("exit", str(dev)))

    def current_stream(dev=None):
        log.append(("current_stream", str(dev)))
        return SimpleNamespace(cuda_stream=1234)

    monkeypatch.setattr(torch.cuda, "device", device)
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: pytest.fail("torch.cuda.synchronize reached"))
    monkeypatch.setattr(torch.cuda, "init", lambda *a, **k: pytest.fail("torch.cuda.init reached"))
    monkeypatch.setattr(torch.cuda, "_lazy_init", lambda *a, **k: pytest.fail("torch.cuda._lazy_init reached"))
    return log


def test_scope_order(no_gpu):
    from sosrt.main import _on_torch_stream
    s = FakeHandle()
    with _on_torch_stream(s, 3) as dev:
        assert str(dev) == "cuda:3"
        assert s.calls == [("set_stream", 1234)] and no_gpu == [("enter", "cuda:3"), ("current_stream", "cuda:3")]
    assert s.calls == [("set_stream", 1234), ("synchronize",), ("set_stream", None)]
    assert no_gpu[-1] == ("exit", "cuda:3")


def test_a_failing_drain_still_puts_the_handle_back(no_gpu):
    from sosrt.main import _on_torch_stream
    boom = RuntimeError("hipErrorLaunchFailure in the drain")
    s = FakeHandle(drain_error=boom)
    with pytest.raises(RuntimeError) as e:
        with _on_torch_stream(s, 0):
            pass
    assert e.value is boom                                    # the original error, not one of the cleanup's
    assert s.calls == [("set_stream", 1234), ("synchronize",), ("set_stream", None)]


def test_an_error_in_the_body_propagates_after_the_drain(no_gpu):
    from sosrt.main import _on_torch_stream
    s = FakeHandle()
    with pytest.raises(KeyError, match="body"):
        with _on_torch_stream(s, 0):
            raise KeyError("body")
    assert s.calls == [("set_stream", 1234), ("synchronize",), ("set_stream", None)]
    # both fail: the handle is still put back, and the drain's error carries the body's as its context
    s = FakeHandle(drain_error=RuntimeError("drain"))
    with pytest.raises(RuntimeError, match="drain") as e:
        with _on_torch_stream(s, 0):
            raise KeyError("body")
    assert isinstance(e.value.__context__, KeyError)
    assert s.calls[-1] == ("set_stream", None)
