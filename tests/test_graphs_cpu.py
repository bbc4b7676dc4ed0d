"""pvpuformer_amd.graphs keeps Python's cyclic collector off while a stream captures (a collection mid-capture runs the destructors
of dead graphs and pools, which call into the runtime): the context that does it, without a GPU."""
import gc

import pytest

from pvpuformer_amd.graphs import _CollectorOff


class _Probe:
    def __init__(self, fail=None):
        self.inside, self.fail = None, fail

    def __enter__(self):
        self.inside = gc.isenabled()
        if self.fail == "enter":
            raise RuntimeError("enter")

    def __exit__(self, *exc):
        if self.fail == "exit":
            raise RuntimeError("exit")


def test_collector_is_off_inside_and_back_on_after():
    assert gc.isenabled()
    dead = []

    class Node:
        def __del__(self):
            dead.append(1)

    a, b = Node(), Node()
    a.other, b.other = b, a                 # a dead cycle: only the cyclic collector frees it
    del a, b
    p = _Probe()
    with _CollectorOff(p):
        assert len(dead) == 2               # collected before the capture begins
        assert p.inside is False and not gc.isenabled()
        with _CollectorOff(_Probe()):       # nested: stays off, and off when the inner one ends
            pass
        assert not gc.isenabled()
    assert gc.isenabled()


@pytest.mark.parametrize("fail", ["enter", "exit", "body"])
def test_collector_comes_back_on_after_an_error(fail):
    with pytest.raises(RuntimeError):
        with _CollectorOff(_Probe(fail)):
            if fail == "body":
                raise RuntimeError("body")
    assert gc.isenabled()


def test_a_collector_the_caller_switched_off_stays_off():
    gc.disable()
    try:
        with _CollectorOff(_Probe()):
            assert not gc.isenabled()
        assert not gc.isenabled()
    finally:
        gc.enable()
