"""GPU test (MI355X) of the FUNCTIONS dispatch path with the HBM state KV:
two back-to-back batches of 48 bench/kvtouch functions through the planner
on one worker, then State.syncAll. 48 is past the batch size (32) at which
the scheduler used to switch dispatch strategy, and several tasks per CPU."""

import pytest

from faabric_amd import _core
from faabric_amd.runtime import LocalRuntime, wait_for_batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

BATCH = 48
KV_BYTES = 4096
KV_SIZE = 1024 * 1024
PAGE = 4096


@pytest.fixture(scope="module")
def runtime():
    rt = LocalRuntime(slots=BATCH, port_offset=13700,
                      planner_port_offset=13700)
    rt.start_planner(with_snapshot_server=False)
    rt.start_worker()
    _core.register_bench_functions()
    # bench/kvtouch uses one process-wide KV: a copy left by an earlier
    # module has that module's (stopped) worker as its master
    _core.state_clear_all()
    yield rt
    _core.state_clear_all()
    rt.stop()


def stats():
    s = _core._debug_kv_commit_stats()
    return int(s["launches"]), int(s["pages"])


def kvtouch_page(msg_id):
    # The page bench/kvtouch writes for this message id (its chunk is one
    # page-aligned page)
    offset = ((msg_id & 0xFFFFFFFF) * 4096) % (KV_SIZE - KV_BYTES)
    assert offset % PAGE == 0
    return offset // PAGE


@requires_gpu
def test_two_kvtouch_batches_commit_every_dirty_page(runtime):
    # Bring the KV into being and drain whatever is pending on it
    _core.state_get_kv_device("bench", "kv", KV_SIZE)
    _core.state_sync_all()
    launches0, pages0 = stats()

    dirtied = set()
    for _ in range(2):
        ber = _core.batch_exec_factory("bench", "kvtouch", BATCH)
        msgs = ber.messages
        for m in msgs:
            m.input_data = b"kvbytes=%d" % KV_BYTES
        ber.messages = msgs
        decision = _core.call_functions(ber)
        assert decision.app_id == ber.app_id
        results = wait_for_batch(ber.app_id, BATCH, timeout_ms=30_000)
        assert len(results) == BATCH
        assert [m.return_value for m in results] == [0] * BATCH
        dirtied.update(kvtouch_page(m.id) for m in ber.messages)

    _core.state_sync_all()
    launches1, pages1 = stats()
    assert launches1 > launches0
    # Nothing synced between the batches, so each dirtied page is listed
    # once (a page two messages share is one dirty bit)
    assert pages1 - pages0 == len(dirtied)
    # A second sync finds nothing left to commit
    _core.state_sync_all()
    assert stats() == (launches1, pages1)
