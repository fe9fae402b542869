"""GPU tests (MI355X) for the device-KV deferred commit: chunk writes land
in the pinned mirror and a dirty bitmap, and sync() commits the dirty
pages to HBM with one scatter-kernel launch. HBM is read back with a
kernel (never through the mirror) and compared whole against a numpy
model of the value."""

import threading

import numpy as np
import pytest

from faabric_amd import _core
from faabric_amd.runtime import LocalRuntime

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

PAGE = 4096
DTYPE_BYTE = 5
OP_SUM = 0


@pytest.fixture(scope="module")
def runtime():
    rt = LocalRuntime(slots=8, port_offset=13500, planner_port_offset=13500)
    rt.start_planner(with_snapshot_server=False)
    rt.start_worker()
    yield rt
    rt.stop()


def read_hbm(ptr, n):
    """Whole value as numpy bytes, read from HBM by a kernel: out = 0 + hbm"""
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _core.device_elementwise_op(out.data_ptr(), ptr, n, DTYPE_BYTE, OP_SUM)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def write(kv, model, offset, data):
    kv.set_chunk(offset, bytes(data))
    model[offset:offset + len(data)] = np.frombuffer(bytes(data), np.uint8)


def stats():
    s = _core._debug_kv_commit_stats()
    return int(s["launches"]), int(s["pages"])


@requires_gpu
def test_commit_odd_geometry(runtime):
    """A value whose last page is partial with a tail that is no multiple
    of 16 bytes; writes straddling a page boundary, the 64 KiB stripe-block
    boundary, and reaching the value's last byte."""
    n = 2 * 65536 + 4096 + 52
    kv = _core.state_get_kv_device("kvcommit", "odd", n)
    model = np.zeros(n, dtype=np.uint8)

    write(kv, model, PAGE * 3 - 4, bytes(range(1, 9)))  # page 2|3
    write(kv, model, 65536 - 100, bytes([0xA5]) * 200)  # stripe block 0|1
    write(kv, model, n - 40, bytes(range(200, 240)))  # up to the last byte
    kv.sync()
    got = read_hbm(kv.data_ptr, n)
    assert np.array_equal(got, model)

    # The whole value, partial tail page included, through one sync
    full = (np.arange(n, dtype=np.uint32) * 7 + 3).astype(np.uint8)
    write(kv, model, 0, full.tobytes())
    kv.sync()
    got = read_hbm(kv.data_ptr, n)
    assert np.array_equal(got, model)


@requires_gpu
def test_commit_writes_only_dirty_pages(runtime):
    """sync() must not rewrite pages nobody wrote through the KV: bytes a
    kernel put straight into HBM on a clean page survive the commit."""
    n = 16 * PAGE
    page_a, page_b = 3, 9
    kv = _core.state_get_kv_device("kvcommit", "dirtyonly", n)
    kv.set(bytes([0x11]) * n)
    ptr = kv.data_ptr  # syncs and invalidates the mirror
    model = np.full(n, 0x11, dtype=np.uint8)

    write(kv, model, page_a * PAGE, bytes([0x77]) * PAGE)
    add = torch.full((PAGE,), 0x22, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _core.device_elementwise_op(ptr + page_b * PAGE, add.data_ptr(), PAGE,
                                DTYPE_BYTE, OP_SUM)
    torch.cuda.synchronize()
    model[page_b * PAGE:(page_b + 1) * PAGE] = 0x33

    kv.sync()
    got = read_hbm(ptr, n)
    assert np.array_equal(got, model)


@requires_gpu
def test_commit_one_launch_per_sync(runtime):
    n = 1024 * 1024
    kv = _core.state_get_kv_device("kvcommit", "onelaunch", n)
    model = np.zeros(n, dtype=np.uint8)
    kv.sync()
    launches0, pages0 = stats()
    for i in range(128):
        page = (i * 2 + 1) % 256
        write(kv, model, page * PAGE, bytes([i + 1]) * PAGE)
    assert stats() == (launches0, pages0)  # nothing committed before sync
    kv.sync()
    assert stats() == (launches0 + 1, pages0 + 128)
    kv.sync()
    assert stats() == (launches0 + 1, pages0 + 128)
    got = read_hbm(kv.data_ptr, n)
    assert np.array_equal(got, model)


@requires_gpu
def test_commit_many_bitmap_words(runtime):
    """8 MiB value = 2048 pages = 32 bitmap words; every other page is
    written, so every word contributes to the one launch."""
    n = 8 * 1024 * 1024
    kv = _core.state_get_kv_device("kvcommit", "manywords", n)
    model = np.zeros(n, dtype=np.uint8)
    kv.sync()
    launches0, pages0 = stats()
    for page in range(0, 2048, 2):
        write(kv, model, page * PAGE, bytes([(page // 2) % 251 + 1]) * PAGE)
    kv.sync()
    assert stats() == (launches0 + 1, pages0 + 1024)
    got = read_hbm(kv.data_ptr, n)
    assert np.array_equal(got, model)


@requires_gpu
def test_commit_concurrent_writers(runtime):
    """Writers race sync(): a page the commit kernel read mid-write has its
    bit set again by its writer, so the final sync() leaves HBM whole."""
    n_threads, pages_each = 16, 4
    n = n_threads * pages_each * PAGE
    kv = _core.state_get_kv_device("kvcommit", "concurrent", n)
    model = np.zeros(n, dtype=np.uint8)
    for t in range(n_threads):
        lo = t * pages_each * PAGE
        model[lo:lo + pages_each * PAGE] = 0x40 + t

    errors = []

    def writer(t):
        try:
            payload = bytes([0x40 + t]) * PAGE
            for p in range(pages_each):
                kv.set_chunk((t * pages_each + p) * PAGE, payload)
        except Exception as e:  # surfaced by the assert below
            errors.append(e)

    threads = [threading.Thread(target=writer, args=(t,))
               for t in range(n_threads)]
    for th in threads:
        th.start()
    while any(th.is_alive() for th in threads):
        kv.sync()
    for th in threads:
        th.join()
    assert not errors, errors
    kv.sync()
    got = read_hbm(kv.data_ptr, n)
    assert np.array_equal(got, model)
