"""amdrec._lib.Gate without a GPU: who may serve and who may capture, by thread (tests/test_threads_gpu.py has the
recommender's side of it)."""
import threading

import pytest

from amdrec import _lib


def _in_thread(fn):
    box = []

    def body():
        try:
            box.append(fn())
        except BaseException as e:                                   # noqa: BLE001
            box.append(e)
    th = threading.Thread(target=body, daemon=True)
    th.start()
    th.join(30)
    assert not th.is_alive() and box
    return box[0]


def _enter(scope):
    with scope():
        return "entered"


def test_serving_nests_and_threads_serve_side_by_side():
    gate = _lib.Gate()
    with gate.serving(), gate.serving():
        assert _in_thread(lambda: _enter(gate.serving)) == "entered"
    assert not gate._calls


def test_capture_and_other_threads_calls_refuse_each_other_without_waiting():
    gate = _lib.Gate()
    with gate.serving():
        assert isinstance(_in_thread(lambda: _enter(gate.capturing)), _lib.AmdrecError)
        assert _enter(gate.capturing) == "entered"                    # the serving thread itself may capture (warm-up calls)
    with gate.capturing():
        assert isinstance(_in_thread(lambda: _enter(gate.serving)), _lib.AmdrecError)
        assert isinstance(_in_thread(lambda: _enter(gate.capturing)), _lib.AmdrecError)
        assert _enter(gate.serving) == "entered" and _enter(gate.capturing) == "entered"
        assert gate._capturer == threading.get_ident()                # (the nested capture's exit did not end the outer one)
    assert gate._capturer is None and not gate._calls
    assert _in_thread(lambda: _enter(gate.capturing)) == "entered"


def test_a_call_that_raises_leaves_the_gate_as_it_was():
    gate = _lib.Gate()
    for scope in (gate.serving, gate.capturing):
        with pytest.raises(ZeroDivisionError):
            with scope():
                1 / 0
    assert not gate._calls and gate._capturer is None and gate._capture_depth == 0
    assert _in_thread(lambda: _enter(gate.capturing)) == "entered"


def test_the_enqueue_lock_is_reentrant_and_exclusive():
    gate = _lib.Gate()
    with gate.enqueue, gate.enqueue:
        assert _in_thread(lambda: gate.enqueue.acquire(blocking=False)) is False
    assert _in_thread(lambda: gate.enqueue.acquire(blocking=False)) is True
