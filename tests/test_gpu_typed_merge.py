"""GPU tests (MI355X): typed merge regions over HBM snapshots. The typed diff
and apply kernels (famTypedDiff, famApplyTypedElems), the TypedElems wire
form, DeviceSnapshot.diff_with_regions and the THREADS fork-join that rides
them, against the numpy models of typed_merge_models.py.

Entries are sorted by index and compared as raw bits. The one exception is
that of test_gpu_kernels.py: a Sum, Subtract or Product value whose model
value is NaN must be NaN at that position.
"""

import multiprocessing as mp
import os
import struct
import sys
import threading
import time

import numpy as np
import pytest

import kernel_models as km
import typed_merge_models as tm
from faabric_amd import _core
from faabric_amd.runtime import LocalRuntime, wait_for_batch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE = tm.PAGE
GUARD = 64  # guard elements on each side of an applied region

DT = {
    tm.T_INT: _core.SnapshotDataType.Int,
    tm.T_LONG: _core.SnapshotDataType.Long,
    tm.T_FLOAT: _core.SnapshotDataType.Float,
    tm.T_DOUBLE: _core.SnapshotDataType.Double,
}
OP = {
    tm.M_SUM: _core.SnapshotMergeOperation.Sum,
    tm.M_SUBTRACT: _core.SnapshotMergeOperation.Subtract,
    tm.M_PRODUCT: _core.SnapshotMergeOperation.Product,
    tm.M_MAX: _core.SnapshotMergeOperation.Max,
    tm.M_MIN: _core.SnapshotMergeOperation.Min,
}
TYPED_ELEMS = _core.SnapshotMergeOperation.TypedElems
XOR_PAGES = _core.SnapshotMergeOperation.XorPages

DIFF_COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
APPLY_COUNTS = [1, 64, 65, 1025]


def _round_up(n, to):
    return (n + to - 1) // to * to


def _noise(nbytes, seed):
    return np.random.default_rng(seed).integers(0, 256, nbytes,
                                                dtype=np.uint8)


def _snapshot_of(host):
    snap = _core.DeviceSnapshot(host.size)
    snap.copy_in_host(host.tobytes())
    return snap


def _snapshot_bytes(snap):
    return np.frombuffer(snap.copy_out_host(snap.size), dtype=np.uint8)


def _typed_elems_diff(dtype, offset, data):
    d = _core.SnapshotDiff()
    d.data_type = DT[dtype]
    d.operation = TYPED_ELEMS
    d.offset = offset
    d.data = data
    return d


def _check_typed_diff(snap, base, dtype, op, start, orig, cur_vals, trailing,
                      what):
    """One typed_diff of the region at `start` holding `orig` in the snapshot
    and `cur_vals` in the arena; every byte outside the region differs."""
    dt = tm.NP_DTYPE[dtype]
    nbytes = orig.size * dt.itemsize
    cur = base ^ np.uint8(0xFF)
    cur[start:start + nbytes] = cur_vals.view(np.uint8)
    cur_dev = km.to_device(cur)
    assert cur_dev.data_ptr() % 16 == 0
    torch.cuda.synchronize()

    got = snap.typed_diff(cur_dev.data_ptr(), start, nbytes + trailing,
                          DT[dtype], OP[op])

    idx, val = tm.typed_diff_model(dtype, op, orig, cur_vals)
    if idx.size == 0:
        assert got is None, what
    else:
        assert got is not None, what
        assert got.operation == TYPED_ELEMS and got.data_type == DT[dtype]
        assert got.offset == start, what
        got_op, got_idx, got_val = tm.unpack_typed_elems(dtype, got.data)
        assert got_op == op, what
        assert got_idx.size == idx.size, what
        got_idx, got_val = tm.sort_entries(got_idx, got_val)
        assert np.array_equal(got_idx, idx), what
        tm.assert_values_equal(dtype, op, got_val, val, what)
    # snap and cur are read only
    assert np.array_equal(_snapshot_bytes(snap), base), what + " snapshot"
    assert np.array_equal(km.to_host(cur_dev), cur), what + " arena"


@requires_gpu
@pytest.mark.parametrize("case", tm.CASES, ids=tm.case_id)
def test_typed_diff(case):
    """famTypedDiff at the chunk, 16 B-line and wave-geometry edges: region
    starts at a page start, one element in, and one element before a page
    end (unaligned head, page crossing)."""
    dtype, op = case
    dt = tm.NP_DTYPE[dtype]
    item = dt.itemsize
    arena = _round_up(PAGE + max(DIFF_COUNTS) * item, PAGE)
    noise = _noise(arena, 21)
    snap = _core.DeviceSnapshot(arena)
    for count in DIFF_COUNTS:
        orig, changed = tm.device_operands(dtype, op, count)
        for start in (0, item, PAGE - item):
            # bytes after the last whole element are diffed by nothing; a
            # count of 0 needs them (length 0 means "to the arena's end")
            trailing = item - 1 if (count == 0 or start == item) else 0
            base = noise.copy()
            base[start:start + count * item] = orig.view(np.uint8)
            snap.copy_in_host(base.tobytes())
            for pattern in tm.CHANGE_PATTERNS:
                if count == 0 and pattern != "none":
                    continue
                _check_typed_diff(
                    snap, base, dtype, op, start, orig,
                    tm.patterned(orig, changed, pattern), trailing,
                    "%s n=%d start=%d %s" % (tm.case_id(case), count, start,
                                             pattern))


@requires_gpu
@pytest.mark.parametrize("dtype", (tm.T_FLOAT, tm.T_DOUBLE),
                         ids=tm.DTYPE_NAME.get)
def test_typed_diff_nan_original_counts_as_changed(dtype):
    """A NaN compares unequal to itself: an element that holds the same NaN
    bits on both sides is still shipped, as the host diff does."""
    dt = tm.NP_DTYPE[dtype]
    count = 257
    orig = np.arange(count).astype(dt)
    orig[[0, 5, 64, 255, 256]] = np.nan
    arena = _round_up(PAGE + count * dt.itemsize, PAGE)
    for op in (tm.M_SUM, tm.M_MAX):
        for start in (0, PAGE - dt.itemsize):
            base = _noise(arena, 22)
            base[start:start + orig.nbytes] = orig.view(np.uint8)
            snap = _snapshot_of(base)
            _check_typed_diff(snap, base, dtype, op, start, orig,
                              orig.copy(), 0, "nan original start=%d" % start)


@requires_gpu
@pytest.mark.parametrize("dtype", tm.TYPED_DTYPES, ids=tm.DTYPE_NAME.get)
def test_product_diff_with_zero_original_raises(dtype):
    dt = tm.NP_DTYPE[dtype]
    for count, zero_at in ((1, 0), (1025, 700)):
        orig = np.full(count, 2, dtype=dt)
        orig[zero_at] = 0
        cur = orig.copy()
        cur[zero_at] = 6
        with pytest.raises(tm.ZeroOriginal):
            tm.typed_diff_model(dtype, tm.M_PRODUCT, orig, cur)
        base = _noise(_round_up(orig.nbytes, PAGE), 23)
        base[:orig.nbytes] = orig.view(np.uint8)
        now = base.copy()
        now[:orig.nbytes] = cur.view(np.uint8)
        snap = _snapshot_of(base)
        cur_dev = km.to_device(now)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="zero original"):
            snap.typed_diff(cur_dev.data_ptr(), 0, orig.nbytes, DT[dtype],
                            OP[tm.M_PRODUCT])
        # a zero original that did not change is no error
        same_dev = km.to_device(base)
        torch.cuda.synchronize()
        assert snap.typed_diff(same_dev.data_ptr(), 0, orig.nbytes,
                               DT[dtype], OP[tm.M_PRODUCT]) is None


@requires_gpu
@pytest.mark.parametrize("case", tm.CASES, ids=tm.case_id)
def test_apply_typed_diff(case):
    """famApplyTypedElems on every other element of a guarded region, in a
    shuffled order; then two malformed diffs that must change nothing."""
    dtype, op = case
    dt = tm.NP_DTYPE[dtype]
    item = dt.itemsize
    offset = GUARD * item
    for count in APPLY_COUNTS:
        target, val = km.operands(tm.KM_DTYPE[dtype], tm.KM_OP[op], count)
        region = np.resize(target[::-1], 2 * count).astype(dt)
        idx = np.random.default_rng(count).permutation(count) * 2
        region[idx] = target
        arena = _round_up(offset + region.nbytes + GUARD * item, PAGE)
        base = _noise(arena, 31)
        base[offset:offset + region.nbytes] = region.view(np.uint8)
        snap = _snapshot_of(base)

        snap.apply_typed_diff(_typed_elems_diff(
            dtype, offset, tm.pack_typed_elems(dtype, op, idx, val)))

        what = "%s n=%d" % (tm.case_id(case), count)
        out = _snapshot_bytes(snap)
        end = offset + region.nbytes
        assert np.array_equal(out[:offset], base[:offset]), what + " low guard"
        assert np.array_equal(out[end:], base[end:]), what + " high guard"
        want = tm.typed_apply_model(dtype, op, region, idx, val)
        tm.assert_values_equal(dtype, op, out[offset:end].copy().view(dt),
                               want, what)

        # one index past the snapshot; a buffer four bytes too long
        past = idx.copy()
        past[count // 2] = (arena - offset) // item
        bad = [tm.pack_typed_elems(dtype, op, past, val),
               tm.pack_typed_elems(dtype, op, idx, val) + b"\x00" * 4]
        for data in bad:
            with pytest.raises(RuntimeError):
                snap.apply_typed_diff(_typed_elems_diff(dtype, offset, data))
            assert np.array_equal(_snapshot_bytes(snap), out), what


def _region_tuple(offset, length, dtype, op):
    return (offset, length, int(DT[dtype].value), int(OP[op].value))


def _parse_xor_pages(diff):
    assert diff.operation == XOR_PAGES
    assert diff.data_type == _core.SnapshotDataType.Raw and diff.offset == 0
    data = diff.data
    (n,) = struct.unpack_from("<I", data, 0)
    assert len(data) == 4 + 4 * n + n * PAGE
    pages = list(struct.unpack_from("<%dI" % n, data, 4))
    payload = np.frombuffer(data, dtype=np.uint8, offset=4 + 4 * n)
    return pages, payload.reshape(n, PAGE)


@requires_gpu
def test_two_arenas_add_to_the_same_elements():
    """Two executors restore one snapshot and both add to the same i32 and
    f32 accumulators: the queued typed diffs merge to s + dA + dB in either
    arrival order, where an XOR merge of the same arenas does not."""
    n = 32
    s_i = (100 + np.arange(64)).astype("<i4")
    s_f = (100 + np.arange(64)).astype("<f4")  # integers, exact in f32
    d_a = np.zeros(64, dtype=np.int64)
    d_b = np.zeros(64, dtype=np.int64)
    d_a[:n] = np.arange(n) + 1
    d_b[:n] = 2 * np.arange(n) + 3

    def arena_with(delta):
        a = np.zeros(2 * PAGE, dtype=np.uint8)
        a[0:256] = (s_i + delta).astype("<i4").view(np.uint8)
        a[256:512] = (s_f + delta).astype("<f4").view(np.uint8)
        return a

    s, a, b = arena_with(0), arena_with(d_a), arena_with(d_b)
    want = arena_with(d_a + d_b)
    regions = [_region_tuple(0, 256, tm.T_INT, tm.M_SUM),
               _region_tuple(256, 256, tm.T_FLOAT, tm.M_SUM)]

    snap = _snapshot_of(s)
    a_dev, b_dev = km.to_device(a), km.to_device(b)
    torch.cuda.synchronize()
    diffs_a = snap.diff_with_regions(a_dev.data_ptr(), regions)
    diffs_b = snap.diff_with_regions(b_dev.data_ptr(), regions)
    for diffs in (diffs_a, diffs_b):
        assert [d.operation for d in diffs][:2] == [TYPED_ELEMS] * 2
        assert [d.offset for d in diffs][:2] == [0, 256]

    for first, second in ((diffs_a, diffs_b), (diffs_b, diffs_a)):
        merged = _snapshot_of(s)
        for d in first + second:
            merged.queue_diff(d)
        assert merged.apply_queued_diffs() == len(first) + len(second)
        assert np.array_equal(_snapshot_bytes(merged), want)
        assert merged.apply_queued_diffs() == 0

    xor_merge = s ^ (s ^ a) ^ (s ^ b)
    assert not np.array_equal(xor_merge, want)
    assert not np.array_equal(xor_merge[:256], want[:256])
    assert not np.array_equal(xor_merge[256:512], want[256:512])


@requires_gpu
def test_mixed_typed_and_raw_pages():
    """A partly typed page, a wholly typed page, a raw page and a clean one."""
    regions_model = [(64, 40, tm.T_INT, tm.M_SUM),
                     (PAGE, PAGE, tm.T_DOUBLE, tm.M_MAX)]
    regions = [_region_tuple(*r) for r in regions_model]
    base = _noise(4 * PAGE, 41)
    ints = (1000 * np.arange(10)).astype("<i4")
    dbls = np.linspace(-50.0, 50.0, PAGE // 8).astype("<f8")
    base[64:104] = ints.view(np.uint8)
    base[PAGE:2 * PAGE] = dbls.view(np.uint8)

    cur = base.copy()
    ints2 = ints.copy()
    ints2[[0, 3, 9]] += np.array([7, -2000, 1], dtype="<i4")
    dbls2 = dbls.copy()
    dbls2[::5] += 3.25   # larger: the maximum moves
    dbls2[1::7] -= 9.5   # smaller: shipped, the merge keeps the target
    cur[64:104] = ints2.view(np.uint8)
    cur[PAGE:2 * PAGE] = dbls2.view(np.uint8)
    cur[0:64] ^= 0xA5
    cur[200:300] ^= 0x3C
    cur[2 * PAGE + 1000:2 * PAGE + 1010] ^= 0xFF

    typed, pages, payload = tm.diff_with_regions_model(base, cur,
                                                       regions_model)
    assert len(typed) == 2 and pages == [0, 2]

    snap = _snapshot_of(base)
    cur_dev = km.to_device(cur)
    torch.cuda.synchronize()
    diffs = snap.diff_with_regions(cur_dev.data_ptr(), regions)
    assert [d.operation for d in diffs] == [TYPED_ELEMS, TYPED_ELEMS,
                                            XOR_PAGES]
    for d, (off, dtype, op, idx, val) in zip(diffs[:2], typed):
        assert d.offset == off and d.data_type == DT[dtype]
        got_op, got_idx, got_val = tm.unpack_typed_elems(dtype, d.data)
        got_idx, got_val = tm.sort_entries(got_idx, got_val)
        assert got_op == op and np.array_equal(got_idx, idx)
        tm.assert_values_equal(dtype, op, got_val, val)
    got_pages, got_payload = _parse_xor_pages(diffs[2])
    assert sorted(got_pages) == [0, 2] and len(got_pages) == 2
    for p, row in zip(got_pages, got_payload):
        assert np.array_equal(row, payload[pages.index(p)]), "page %d" % p
    page0 = got_payload[got_pages.index(0)]
    assert not page0[64:104].any()
    assert page0[0:64].all() and page0[200:300].all()
    assert np.array_equal(_snapshot_bytes(snap), base)

    second = _snapshot_of(base)
    for d in diffs:
        second.queue_diff(d)
    assert second.apply_queued_diffs() == 3
    want = tm.apply_region_diffs_model(base, typed, pages, payload)
    assert np.array_equal(_snapshot_bytes(second), want)
    # the raw bytes and the summed ints arrive; the maxima are the model's
    assert np.array_equal(want[:PAGE], cur[:PAGE])
    assert not np.array_equal(want[PAGE:2 * PAGE], cur[PAGE:2 * PAGE])

    # regions the device path cannot honour
    for bad in ([(0, 32, int(_core.SnapshotDataType.Bool.value),
                  int(OP[tm.M_SUM].value))],
                [_region_tuple(2, 32, tm.T_INT, tm.M_SUM)],
                [_region_tuple(0, 64, tm.T_INT, tm.M_SUM),
                 _region_tuple(32, 64, tm.T_FLOAT, tm.M_SUM)],
                [(0, 32, int(DT[tm.T_INT].value), int(TYPED_ELEMS.value))]):
        with pytest.raises(RuntimeError):
            snap.diff_with_regions(cur_dev.data_ptr(), bad)


# ---------------------------------------------------------------------------
# THREADS fork-join
# ---------------------------------------------------------------------------

FORK_PAGES = 4
INT_SUM = (int(_core.SnapshotDataType.Int.value),
           int(_core.SnapshotMergeOperation.Sum.value))
FLOAT_SUM = (int(_core.SnapshotDataType.Float.value),
             int(_core.SnapshotMergeOperation.Sum.value))


@pytest.fixture
def runtime():
    rt = LocalRuntime(slots=8, port_offset=13900, planner_port_offset=13900)
    rt.start_planner(with_snapshot_server=False)
    rt.start_worker()
    yield rt
    rt.stop()


def _counter_thread_body(msg):
    # Thread i adds i to its own counter and flips a raw byte in the same
    # page as the typed region
    idx = msg.group_idx
    (v,) = struct.unpack(
        "<i", _core.executor_device_read_memory((idx - 1) * 4, 4))
    _core.executor_device_write_memory((idx - 1) * 4,
                                       struct.pack("<i", v + idx))
    (raw,) = _core.executor_device_read_memory(64 + idx, 1)
    _core.executor_device_write_memory(64 + idx, bytes([raw ^ 0xFF]))
    return 0


def _counter_fork_parent(msg):
    size = FORK_PAGES * PAGE
    _core.executor_set_device_memory_size(size)
    base = bytearray([0x30]) * size
    base[0:32] = struct.pack("<8i", *([100] * 8))
    _core.executor_device_write_memory(0, bytes(base))

    bool_type = int(_core.SnapshotDataType.Bool.value)
    for bad in ((0, 32, bool_type, INT_SUM[1]), (2, 32) + INT_SUM):
        try:
            _core.execute_threads("typedmerge", "body", 3,
                                  merge_regions=[bad])
        except RuntimeError:
            continue
        msg.output_data = "region %r was accepted" % (bad,)
        return 4

    results = _core.execute_threads(
        "typedmerge", "body", 3, merge_regions=[(0, 32) + INT_SUM])
    if len(results) != 3 or any(rv != 0 for _, rv in results):
        msg.output_data = "thread failures: %r" % (results,)
        return 1

    data = _core.executor_device_read_memory(0, size)
    want = bytearray(base)
    want[0:32] = struct.pack("<8i", 101, 102, 103, 100, 100, 100, 100, 100)
    for i in (1, 2, 3):
        want[64 + i] ^= 0xFF
    if data[0:32] != bytes(want[0:32]):
        msg.output_data = "counters: %r" % (struct.unpack("<8i", data[0:32]),)
        return 2
    if data != bytes(want):
        bad_at = [i for i in range(size) if data[i] != want[i]][:8]
        msg.output_data = "bytes differ at %r" % (bad_at,)
        return 3
    msg.output_data = "typed fork-join ok"
    return 0


@requires_gpu
def test_fork_join_with_a_sum_region(runtime):
    """THREADS fork-join on one worker: eight i32 counters under an Int Sum
    region, raw byte edits in the same page, and two regions that the
    parent's call must reject."""
    _core.register_function("typedmerge", "body", _counter_thread_body)
    _core.register_function("typedmerge", "parent", _counter_fork_parent)
    ber = _core.batch_exec_factory("typedmerge", "parent", 1)
    decision = _core.call_functions(ber)
    assert decision.app_id == ber.app_id
    results = wait_for_batch(ber.app_id, 1, timeout_ms=60_000)
    parent = [r for r in results if r.output_data][0]
    assert parent.return_value == 0, parent.output_data
    assert parent.output_data == "typed fork-join ok"


DIST_PLANNER_OFFSET = 14500
DIST_WORKER_OFFSETS = (14100, 14300)
DIST_WORKER_SLOTS = 2
# 1001, not 1000: the XOR merge of the workers' arenas has to differ from the
# sum (1000 ^ 1001 ^ 1002 == 1003, as integers and as f32 bits alike);
# test_xor_merge_cannot_pass_for_the_sum checks the choice
DIST_BASE = 1001
DIST_REGIONS = [(0, 4) + INT_SUM, (4, 4) + FLOAT_SUM]
RV_REGIONS = 100  # a thread returns RV_REGIONS + the regions its host holds

# Threads of one worker share its executor's arena: their read-modify-write
# of the shared counters is serialised per process
_RMW_LOCK = threading.Lock()


def _shared_counter_thread_body(msg):
    with _RMW_LOCK:
        i, f = struct.unpack("<if", _core.executor_device_read_memory(0, 8))
        _core.executor_device_write_memory(0, struct.pack("<if", i + 1,
                                                          f + 1.0))
    # What this host's registry holds for the fork's key while the thread
    # runs: on the remote worker they arrived by RPC ahead of the snapshot
    held = _core.executor_device_merge_regions()
    if held and sorted(held) != sorted(DIST_REGIONS):
        return 1
    return RV_REGIONS + len(held)


def _region_count_thread_body(msg):
    return RV_REGIONS + len(_core.executor_device_merge_regions())


def _shared_counter_fork_parent(msg):
    _core.executor_set_device_memory_size(PAGE)
    base = bytearray([0x30]) * PAGE
    base[0:8] = struct.pack("<if", DIST_BASE, float(DIST_BASE))
    _core.executor_device_write_memory(0, bytes(base))
    results = _core.execute_threads(
        "typedmergedist", "body", 3, merge_regions=DIST_REGIONS)
    # every thread, on either worker, found both regions under the key
    if len(results) != 3 or any(rv != RV_REGIONS + 2 for _, rv in results):
        msg.output_data = "thread results: %r" % (results,)
        return 1
    data = _core.executor_device_read_memory(0, PAGE)
    i, f = struct.unpack("<if", data[0:8])
    if (i, f) != (DIST_BASE + 3, float(DIST_BASE + 3)):
        msg.output_data = "counters: %r %r" % (i, f)
        return 2
    if data[8:] != bytes(base[8:]):
        msg.output_data = "bytes outside the regions changed"
        return 3
    # The join took the regions back, here and on the remote worker: the
    # threads of a fork without regions find none on either host (they
    # leave the memory alone; only their return values are looked at)
    results = _core.execute_threads("typedmergedist", "regioncount", 3)
    if len(results) != 3 or any(rv != RV_REGIONS for _, rv in results):
        msg.output_data = "regions after the join: %r" % (results,)
        return 4
    msg.output_data = "typed dist fork ok"
    return 0


def _xor_bits(dtype, *values):
    out = 0
    for v in values:
        out ^= int(np.array([v], dtype=dtype).view("<u4")[0])
    return out


def test_xor_merge_cannot_pass_for_the_sum():
    """With the three increments split over the two workers (one and two:
    the test asserts that both ran threads), whichever of the two diffs went
    the XOR way, the merged counters differ from base + 3 for the base that
    the two-worker test uses. Plain numpy."""
    s = DIST_BASE
    for dtype in ("<i4", "<f4"):
        want = _xor_bits(dtype, s + 3)
        for a, b in ((1, 2), (2, 1)):
            # both arenas XOR-merged: s ^ (s ^ (s+a)) ^ (s ^ (s+b))
            assert _xor_bits(dtype, s, s + a, s + b) != want, (dtype, a, b)
            # one diff typed (+a), the other an XOR page diff of s+b
            assert _xor_bits(dtype, s + a, s, s + b) != want, (dtype, a, b)
    # the base this test must not use
    assert _xor_bits("<i4", 1000, 1001, 1002) == 1003


def _dist_worker_main(port_offset, stop_event, ready_event):
    sys.path.insert(0, REPO_ROOT)
    from faabric_amd import _core as core
    from faabric_amd.runtime import LocalRuntime as Runtime

    core.set_log_level("error")
    rt = Runtime(port_offset=port_offset,
                 planner_port_offset=DIST_PLANNER_OFFSET,
                 slots=DIST_WORKER_SLOTS)
    rt.start_worker()
    core.register_function("typedmergedist", "body",
                           _shared_counter_thread_body)
    core.register_function("typedmergedist", "regioncount",
                           _region_count_thread_body)
    core.register_function("typedmergedist", "parent",
                           _shared_counter_fork_parent)
    ready_event.set()
    stop_event.wait(120)
    rt.stop()


class _Cluster:
    """The spawned workers, keyed by host identity, each with its own stop
    event."""

    def __init__(self):
        self.workers = {}  # identity -> (process, stop event)
        self.stop_first = None

    def stop(self):
        # The forking worker goes first: it deletes its fork snapshot on its
        # peer as it shuts down, which must not find the peer gone and wait
        # for a connection to it
        order = sorted(self.workers, key=lambda h: h != self.stop_first)
        for host in order:
            proc, stop = self.workers[host]
            stop.set()
            proc.join(timeout=30)
            if proc.is_alive():
                proc.terminate()


@pytest.fixture
def cluster():
    # Planner runs in this process; no worker here
    rt = LocalRuntime(port_offset=DIST_PLANNER_OFFSET,
                      planner_port_offset=DIST_PLANNER_OFFSET)
    rt.start_planner()

    ctx = mp.get_context("spawn")
    cl = _Cluster()
    readies = []
    # Snapshot shipping takes the host-copy path in the workers
    saved = os.environ.get("FAABRIC_IPC_DISABLE")
    os.environ["FAABRIC_IPC_DISABLE"] = "1"
    try:
        for off in DIST_WORKER_OFFSETS:
            ready = ctx.Event()
            stop = ctx.Event()
            p = ctx.Process(target=_dist_worker_main,
                            args=(off, stop, ready))
            p.start()
            cl.workers["127.0.0.1@%d" % off] = (p, stop)
            readies.append(ready)
    finally:
        if saved is None:
            del os.environ["FAABRIC_IPC_DISABLE"]
        else:
            os.environ["FAABRIC_IPC_DISABLE"] = saved
    try:
        for r in readies:
            assert r.wait(120), "worker failed to start"
        deadline = time.monotonic() + 10
        while time.monotonic() < deadline:
            if len(_core.get_available_hosts()) == 2:
                break
            time.sleep(0.05)
        yield cl
    finally:
        cl.stop()
        rt.stop()


@requires_gpu
def test_fork_join_across_two_workers(cluster):
    """Threads on BOTH workers (sharing GPU 0) add to the same i32 and f32
    counters under Sum regions: the regions travel to the remote worker by
    key ahead of the snapshot, its typed diff merges back over the
    ThreadResult channel, and the join takes the regions back on both hosts.
    The base makes every XOR merge of the same arenas give another value."""
    assert len(_core.get_available_hosts()) == 2
    # Parent takes 1 slot on its host; 3 threads need the remaining slot
    # there plus 2 on the other worker
    ber = _core.batch_exec_factory("typedmergedist", "parent", 1)
    decision = _core.call_functions(ber)
    assert decision.app_id == ber.app_id
    # the parent, three counting threads, three threads of the second fork
    results = wait_for_batch(ber.app_id, 7, timeout_ms=60_000)
    parent = [r for r in results if r.output_data][0]
    cluster.stop_first = parent.executed_host
    assert parent.return_value == 0, parent.output_data
    assert parent.output_data == "typed dist fork ok"
    assert len(results) == 7
    first_fork = [r for r in results if r.return_value == RV_REGIONS + 2]
    assert len(first_fork) == 3
    assert len({r.executed_host for r in first_fork}) == 2
    second_fork = [r for r in results if r.return_value == RV_REGIONS]
    assert len(second_fork) == 3
    assert len({r.executed_host for r in second_fork}) == 2
    hosts = {r.executed_host for r in results}
    assert hosts == {"127.0.0.1@%d" % off for off in DIST_WORKER_OFFSETS}
