"""FUNCTIONS batch dispatch and completion: the warm pool's idle list, the
batch claim, the mailbox hand-off to executor threads and the planner's
message-position index. One planner and one worker in this process; the
functions are Python callables so the tests can count what ran where."""

import threading
import time

import pytest

from faabric_amd import _core
from faabric_amd.runtime import LocalRuntime, wait_for_batch

SLOTS = 256
DEFAULT_BOUND_TIMEOUT_MS = 30000

_lock = threading.Lock()
_runs = {}  # message id -> times run
_in_use = set()  # executor ids running a rendezvous function
_violations = []
_gate = threading.Event()


def fn_count(msg):
    with _lock:
        _runs[msg.id] = _runs.get(msg.id, 0) + 1
    return msg.app_idx % 5


def fn_rendezvous(msg):
    eid = _core._debug_current_executor_id()
    with _lock:
        if eid in _in_use:
            _violations.append(eid)
        _in_use.add(eid)
    time.sleep(0.002)
    with _lock:
        _in_use.discard(eid)
    return 0


def fn_reverse(msg):
    # Later messages finish first
    time.sleep((64 - msg.app_idx) * 0.002)
    return 0


def fn_gated(msg):
    _gate.wait(20)
    return 0


def fn_fail(msg):
    raise RuntimeError("boom %d" % msg.app_idx)


def fn_thread(msg):
    _core.executor_write_memory(64 + msg.group_idx, bytes([msg.group_idx]))
    return 0


N_THREADS = 40


def fn_thread_parent(msg):
    _core.executor_set_memory_size(4096)
    _core.executor_write_memory(0, bytes(4096))
    results = _core.execute_threads("dp", "thread", N_THREADS)
    if len(results) != N_THREADS or any(rv != 0 for _, rv in results):
        msg.output_data = f"thread failures: {results}"
        return 1
    got = _core.executor_read_memory(64, N_THREADS + 1)
    if got[1:] != bytes(range(1, N_THREADS + 1)):
        msg.output_data = f"bad merge: {got!r}"
        return 2
    return 0


@pytest.fixture(scope="module")
def runtime():
    rt = LocalRuntime(slots=SLOTS, port_offset=17400,
                      planner_port_offset=17400)
    rt.start_planner(with_snapshot_server=False)
    rt.start_worker()
    _core.register_function("dp", "count", fn_count)
    _core.register_function("dp", "rendezvous", fn_rendezvous)
    _core.register_function("dp", "reverse", fn_reverse)
    _core.register_function("dp", "gated", fn_gated)
    _core.register_function("dp", "fail", fn_fail)
    _core.register_function("dp", "thread", fn_thread)
    _core.register_function("dp", "thread_parent", fn_thread_parent)
    _core.register_native_noop("dp", "noop")
    _core.register_native_noop("dp", "warm")
    _core.register_native_noop("dp", "reap")
    yield rt
    _core.set_bound_timeout(DEFAULT_BOUND_TIMEOUT_MS)
    rt.stop()


def run_batch(function, n, timeout_ms=30_000):
    ber = _core.batch_exec_factory("dp", function, n)
    decision = _core.call_functions(ber)
    assert decision.app_id == ber.app_id, decision.app_id
    results = wait_for_batch(ber.app_id, n, timeout_ms)
    return ber, results


def sizes():
    d = dict(_core._debug_runtime_sizes())
    d.update(_core._debug_dispatch_sizes())
    return {k: int(v) for k, v in d.items()}


def assert_planner_drained():
    s = sizes()
    assert s["planner_in_flight"] == 0, s
    assert s["planner_msg_index_apps"] == 0, s
    assert s["planner_used_slots"] == 0, s


# 32 is where executeBatch used to switch to its fan-out pool
@pytest.mark.parametrize("n", [1, 31, 32, 33, 200])
def test_batch_sizes(runtime, n):
    with _lock:
        _runs.clear()
    ber, results = run_batch("count", n)
    ids = [m.id for m in ber.messages]
    assert len(set(ids)) == n
    with _lock:
        runs = dict(_runs)
    assert runs == {i: 1 for i in ids}
    status = _core.get_batch_results(ber.app_id)
    assert status.finished
    assert len(results) == n
    assert sorted(m.id for m in results) == sorted(ids)
    assert [m.return_value for m in results] == [i % 5 for i in range(n)]
    assert_planner_drained()


def test_warm_reuse(runtime):
    _core.scheduler_reset()
    n = 40
    run_batch("warm", n)
    assert _core.get_executor_count() == n
    assert sizes()["idle_executors"] == n
    run_batch("warm", n)
    assert _core.get_executor_count() == n
    run_batch("warm", n + 5)
    assert _core.get_executor_count() == n + 5
    assert sizes()["idle_executors"] == n + 5


def test_concurrent_batches(runtime):
    del _violations[:]
    done = {}
    errors = []

    def submit(tag):
        try:
            _, results = run_batch("rendezvous", 40)
            done[tag] = results
        except Exception as e:  # surfaced by the assert below
            errors.append(e)

    threads = [threading.Thread(target=submit, args=(t,)) for t in "ab"]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for tag in "ab":
        assert len(done[tag]) == 40
        assert all(m.return_value == 0 for m in done[tag])
    assert _violations == []
    assert_planner_drained()


def test_reaper_against_idle_list(runtime):
    _core.scheduler_reset()
    n = 12
    _core.set_bound_timeout(40)
    try:
        run_batch("reap", n)
        assert _core.get_executor_count() == n
        time.sleep(0.12)
        assert _core.reap_stale_executors() == n
        assert _core.get_executor_count() == 0
        # A reaped executor left the idle list with the pool
        assert sizes()["idle_executors"] == 0
    finally:
        _core.set_bound_timeout(DEFAULT_BOUND_TIMEOUT_MS)
    _, results = run_batch("reap", n)
    assert all(m.return_value == 0 for m in results)
    assert _core.get_executor_count() == n
    assert sizes()["idle_executors"] == n


def test_out_of_order_completion(runtime):
    _, results = run_batch("reverse", 64)
    assert len(results) == 64
    assert all(m.return_value == 0 for m in results)
    finish = [m.finish_timestamp for m in results]
    assert finish[0] >= finish[-1]  # app_idx 0 slept longest
    assert_planner_drained()
    # Slots were released exactly once each: a fresh app that needs every
    # slot of the host is scheduled
    _, results = run_batch("noop", SLOTS)
    assert len(results) == SLOTS
    assert_planner_drained()


def test_duplicate_result(runtime):
    _, first = run_batch("count", 8)
    assert_planner_drained()
    # Hold 4 slots with a second app, so a slot released twice would show
    # (the planner never counts below zero)
    _gate.clear()
    held = _core.batch_exec_factory("dp", "gated", 4)
    try:
        assert _core.call_functions(held).app_id == held.app_id
        assert sizes()["planner_used_slots"] == 4
        _core._debug_set_message_result(first[0])
        _core._debug_set_message_result(first[0])
        time.sleep(0.1)
        assert sizes()["planner_used_slots"] == 4
    finally:
        _gate.set()
    wait_for_batch(held.app_id, 4)
    assert_planner_drained()
    _, results = run_batch("noop", SLOTS)
    assert len(results) == SLOTS


def test_threads_many_tasks_on_one_executor(runtime):
    # More threads than any executor has pool threads on a small host, so
    # pool threads take several tasks each through their mailbox
    _, results = run_batch("thread_parent", 1)
    assert results[0].return_value == 0, results[0].output_data
    assert_planner_drained()


def test_failing_function_releases_executor(runtime):
    _core.scheduler_reset()
    n = 6
    _, results = run_batch("fail", n)
    assert [m.return_value for m in results] == [1] * n
    assert all("boom" in m.output_data for m in results)
    assert _core.get_executor_count() == n
    assert sizes()["idle_executors"] == n
    run_batch("fail", n)
    assert _core.get_executor_count() == n
    assert_planner_drained()
