"""GPU tests (MI355X): every kernel entry point of cpp/hip/snapshot_kernels.hip
against the CPU numpy models of kernel_models.py, at edge values and at the
geometry edges of the launch shapes.

Results are copied to the host and compared as raw bits with no tolerance.
The single exception is a SUM, SUB or PROD whose model result is NaN: the
device result must be NaN at exactly those positions (payload and sign differ
between x86 and the GPU). MAX and MIN are selections and match bit for bit.

Not reachable here: the 2-way unrolled loops of elementwiseOpKernel and
xorBufferKernel. Their grids are one element per lane and have no tunable, so
only the tail loops of those two kernels run.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_models as km
from faabric_amd import _core

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs an MI355X"
)

PAGE = km.PAGE
GUARD = 64  # guard elements on each side of the operated range
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 513]

TYPED_OPS = [km.OP_SUM, km.OP_MAX, km.OP_MIN, km.OP_PROD, km.OP_SUB]
ELEMENTWISE_CASES = [(d, o) for d in sorted(km.NP_DTYPE) for o in TYPED_OPS]
ELEMENTWISE_CASES.append((km.DT_BYTE, km.OP_XOR))


def _case_id(case):
    return "%s-%s" % (km.DTYPE_NAME[case[0]], km.OP_NAME[case[1]])


def _guarded(values, byte_shift, fill_seed):
    """Host bytes of `values` in the middle of a larger allocation: GUARD
    elements of noise on each side, the whole shifted by byte_shift bytes.
    Returns (bytes, offset of the first value)."""
    item = values.dtype.itemsize
    rng = np.random.default_rng(fill_seed)
    lead = GUARD * item + byte_shift
    total = lead + values.size * item + GUARD * item
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    buf[lead:lead + values.size * item] = values.view(np.uint8)
    return buf, lead


def _run_elementwise(dtype, op, n, byte_shift=0):
    dt = km.NP_DTYPE[dtype]
    inout, inp = km.operands(dtype, op, n)
    want = km.elementwise_model(op, dtype, inout, inp)

    a_host, a_off = _guarded(inout, byte_shift, 11)
    b_host, b_off = _guarded(inp, byte_shift, 12)
    a_dev, b_dev = km.to_device(a_host), km.to_device(b_host)
    torch.cuda.synchronize()
    _core.device_elementwise_op(
        a_dev.data_ptr() + a_off, b_dev.data_ptr() + b_off, n, dtype, op)
    a_got, b_got = km.to_host(a_dev), km.to_host(b_dev)

    what = "%s n=%d shift=%d" % (_case_id((dtype, op)), n, byte_shift)
    end = a_off + n * dt.itemsize
    assert np.array_equal(a_got[:a_off], a_host[:a_off]), what + " low guard"
    assert np.array_equal(a_got[end:], a_host[end:]), what + " high guard"
    assert np.array_equal(b_got, b_host), what + " in buffer"
    got = a_got[a_off:end].copy().view(dt)
    km.assert_elementwise_equal(op, dtype, got, want, what)


@requires_gpu
@pytest.mark.parametrize("case", ELEMENTWISE_CASES, ids=_case_id)
def test_elementwise_vs_model(case):
    dtype, op = case
    for n in LENGTHS:
        _run_elementwise(dtype, op, n)


@requires_gpu
@pytest.mark.parametrize(
    "op", TYPED_OPS + [km.OP_XOR], ids=km.OP_NAME.get)
def test_elementwise_bytes_from_unaligned_pointers(op):
    """Both byte kernels claim to be alignment-free."""
    for shift in (1, 3):
        for n in (1, 63, 65, 255, 257, 513):
            _run_elementwise(km.DT_BYTE, op, n, byte_shift=shift)


def test_elementwise_cases_are_complete():
    """All six dtypes x five typed ops, plus byte XOR; at the longest length
    every pairing of the value set is present."""
    assert len(ELEMENTWISE_CASES) == 31 and len(set(ELEMENTWISE_CASES)) == 31
    for dtype, op in ELEMENTWISE_CASES:
        assert km.operand_pairs(dtype, op)[0].size <= max(LENGTHS)


INVALID_CASES = (
    [(d, km.OP_XOR) for d in range(5)]
    + [(d, o) for d in (km.DT_INT32, km.DT_FLOAT, km.DT_BYTE)
       for o in (-1, 6, 100)]
    + [(d, o) for d in (-1, 6, 100) for o in (km.OP_SUM, km.OP_XOR)]
)


@requires_gpu
@pytest.mark.parametrize("case", INVALID_CASES, ids=lambda c: "%d-%d" % c)
def test_elementwise_rejects_invalid_pair(case):
    dtype, op = case
    rng = np.random.default_rng(5)
    a_host = rng.integers(0, 256, 1024, dtype=np.uint8)
    b_host = rng.integers(0, 256, 1024, dtype=np.uint8)
    a_dev, b_dev = km.to_device(a_host), km.to_device(b_host)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        _core.device_elementwise_op(
            a_dev.data_ptr(), b_dev.data_ptr(), 64, dtype, op)
    torch.cuda.synchronize()
    assert np.array_equal(km.to_host(a_dev), a_host)
    assert np.array_equal(km.to_host(b_dev), b_host)


# ---------------------------------------------------------------------------
# Whole-buffer copy and XOR
# ---------------------------------------------------------------------------

MIB = 1 << 20
COPY_SIZES = [0, 16, 4080, 4096, 4112, MIB, MIB + 16, 4099]


@pytest.fixture(scope="module")
def copy_source():
    return km.random_source(MIB + 64)


@requires_gpu
@pytest.mark.parametrize("nbytes", COPY_SIZES)
def test_copy_buffer(copy_source, nbytes):
    """4099 takes the runtime-copy fallback for its size; the offset pointers
    take it for their alignment."""
    src_dev, src_host = copy_source
    for src_off, dst_off in km.COPY_OFFSETS:
        km.check_copy_buffer(nbytes, src_off, dst_off, src_dev, src_host)
    assert np.array_equal(km.to_host(src_dev), src_host)


@requires_gpu
@pytest.mark.parametrize("nbytes", [s for s in COPY_SIZES if s % 16 == 0])
def test_xor_buffer(copy_source, nbytes):
    a_dev, a_host = copy_source
    b_dev, b_host = km.random_source(nbytes + 32, seed=8)
    total = km.COPY_GUARD + nbytes + km.COPY_GUARD
    guard = (np.arange(total, dtype=np.uint32) * 5 + 1).astype(np.uint8)
    out = km.to_device(guard)
    torch.cuda.synchronize()
    # second operand from a 16 B-aligned interior offset
    _core.fam_xor_buffer(a_dev.data_ptr(), b_dev.data_ptr() + 16,
                         out.data_ptr() + km.COPY_GUARD, nbytes)
    want = guard.copy()
    want[km.COPY_GUARD:km.COPY_GUARD + nbytes] = (
        a_host[:nbytes] ^ b_host[16:16 + nbytes])
    assert np.array_equal(km.to_host(out), want)
    assert np.array_equal(km.to_host(a_dev), a_host)
    assert np.array_equal(km.to_host(b_dev), b_host)


@requires_gpu
def test_xor_buffer_rejects_unvectorisable_size(copy_source):
    a_dev, a_host = copy_source
    out_host = np.full(8192, 0xA5, dtype=np.uint8)
    out = km.to_device(out_host)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        _core.fam_xor_buffer(a_dev.data_ptr(), a_dev.data_ptr() + 8192,
                             out.data_ptr(), 4099)
    torch.cuda.synchronize()
    assert np.array_equal(km.to_host(out), out_host)


# ---------------------------------------------------------------------------
# Snapshot geometry
# ---------------------------------------------------------------------------

PAGE_COUNTS = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097]


@requires_gpu
@pytest.mark.parametrize("n_pages", PAGE_COUNTS)
def test_snapshot_geometry(n_pages):
    km.check_snapshot_geometry(n_pages)


def _snapshot_of(base):
    dev = km.to_device(base)
    torch.cuda.synchronize()
    snap = _core.DeviceSnapshot(base.size)
    snap.capture_from_ptr(dev.data_ptr())
    return snap


def _snapshot_bytes(snap):
    return np.frombuffer(snap.copy_out_host(snap.size), dtype=np.uint8)


@requires_gpu
def test_snapshot_component_sweep():
    """Page p differs in one bit of 16-byte vector p, 32-bit word p % 4: all
    four vector words and all four 1 KiB slices a lane loads."""
    n_pages = 256
    rng = np.random.default_rng(21)
    base = rng.integers(0, 256, n_pages * PAGE, dtype=np.uint8)
    upd = base.copy()
    for p in range(n_pages):
        off = p * 16 + (p % 4) * 4 + (p // 4) % 4
        upd[p * PAGE + off] ^= np.uint8(1 << (p % 8))
    words = km.payload_model(base, upd).view("<u4")
    for p in range(n_pages):
        assert np.nonzero(words[p])[0].tolist() == [p * 4 + p % 4]
    km.check_diff(_snapshot_of(base), base, upd, "component sweep")


@requires_gpu
def test_snapshot_object_reuse():
    """A second diff on the same object reports only its own set."""
    n_pages = 2049
    rng = np.random.default_rng(22)
    base = rng.integers(0, 256, n_pages * PAGE, dtype=np.uint8)
    snap = _snapshot_of(base)

    upd1 = base.copy()
    for p in range(0, n_pages, 2):  # 1025 whole pages, every byte differs
        upd1[p * PAGE:(p + 1) * PAGE] ^= np.uint8(0xFF)
    km.check_diff(snap, base, upd1, "reuse: large set")

    # 32 and 2048 were in the first set, 3 and 2047 were not
    upd2 = km.flip_pages(upd1, [3, 32, 2047, 2048])
    km.check_diff(snap, upd1, upd2, "reuse: small set")

    # nothing dirty, then apply: unchanged
    dev = km.to_device(upd2)
    torch.cuda.synchronize()
    assert snap.diff_xor(dev.data_ptr()) == 0
    snap.apply_last_diff()
    assert np.array_equal(_snapshot_bytes(snap), upd2)
    assert not any(snap.dirty_pages(dev.data_ptr()))


@requires_gpu
def test_apply_compact_diff_order_and_validation():
    n_pages = 70
    rng = np.random.default_rng(23)
    base = rng.integers(0, 256, n_pages * PAGE, dtype=np.uint8)
    upd = rng.integers(0, 256, n_pages * PAGE, dtype=np.uint8)
    pages = [0, 5, 31, 32, 33, 63, 64, 69]
    clean = np.setdiff1d(np.arange(n_pages), pages)
    upd.reshape(n_pages, PAGE)[clean] = base.reshape(n_pages, PAGE)[clean]
    payload = km.payload_model(base, upd)

    shuffled = [int(p) for p in rng.permutation(pages)]
    assert shuffled != pages and shuffled != pages[::-1]
    for order in (pages, pages[::-1], shuffled):
        snap = _snapshot_of(base)
        snap.apply_compact_diff(order, payload[order].tobytes())
        assert np.array_equal(_snapshot_bytes(snap), upd), order

    snap = _snapshot_of(base)
    with pytest.raises(RuntimeError):
        snap.apply_compact_diff([0, n_pages], payload[[0, 1]].tobytes())
    assert np.array_equal(_snapshot_bytes(snap), base)
    with pytest.raises(RuntimeError):
        snap.apply_compact_diff([0, 5], payload[[0]].tobytes())
    assert np.array_equal(_snapshot_bytes(snap), base)
    with pytest.raises(RuntimeError):
        snap.apply_compact_diff([0], payload[[0]].tobytes() + b"\x00")
    assert np.array_equal(_snapshot_bytes(snap), base)


@requires_gpu
def test_snapshot_rejects_partial_page_size():
    for size in (1, PAGE - 1, PAGE + 16, 3 * PAGE + 2048):
        with pytest.raises(RuntimeError):
            _core.DeviceSnapshot(size)


# ---------------------------------------------------------------------------
# Bench-input kernels
# ---------------------------------------------------------------------------


@requires_gpu
@pytest.mark.parametrize("n_words", [1, 513, 65537])
def test_fill_random_vs_model(n_words):
    seed = 0xDEADBEEFCAFEF00D
    guard = np.full(n_words + 2 * GUARD, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    dev = km.to_device(guard)
    torch.cuda.synchronize()
    _core.fam_fill_random(dev.data_ptr() + GUARD * 8, n_words * 8, seed)
    want = guard.copy()
    want[GUARD:GUARD + n_words] = km.fill_random_model(n_words, seed)
    assert np.array_equal(km.to_host(dev).view(np.uint64), want)


@requires_gpu
def test_fill_random_rejects_partial_word():
    host = np.full(64, 0x5A, dtype=np.uint8)
    dev = km.to_device(host)
    torch.cuda.synchronize()
    for nbytes in (1, 7, 12, 33):
        with pytest.raises(RuntimeError):
            _core.fam_fill_random(dev.data_ptr(), nbytes, 1)
    torch.cuda.synchronize()
    assert np.array_equal(km.to_host(dev), host)


@requires_gpu
@pytest.mark.parametrize("n_touch", [1, 5, 64])
def test_touch_pages_vs_model(n_touch):
    """64 pages is more than the waves of one block; the list is unsorted."""
    n_pages = 64
    seed = 0x0123456789ABCDEF
    rng = np.random.default_rng(30 + n_touch)
    words = rng.integers(0, 2**64, n_pages * PAGE // 8, dtype=np.uint64)
    pages = [int(p) for p in rng.permutation(n_pages)[:n_touch]]
    if n_touch > 1:
        assert pages != sorted(pages)
    dev = km.to_device(words)
    torch.cuda.synchronize()
    _core.fam_touch_pages(dev.data_ptr(), pages, seed)
    want = km.touch_pages_model(words, pages, seed)
    got = km.to_host(dev).view(np.uint64)
    assert np.array_equal(got, want)
    untouched = np.setdiff1d(np.arange(n_pages), pages)
    assert np.array_equal(got.reshape(n_pages, -1)[untouched],
                          words.reshape(n_pages, -1)[untouched])


# ---------------------------------------------------------------------------
# Tunable paths: grid-stride loops and the other template instantiations
# ---------------------------------------------------------------------------

TUNABLES = {
    "FAM_DIFF_BLOCKS": "2",
    "FAM_APPLY_BLOCKS": "1",
    "FAM_COPY_GRID": "1",
    "FAM_DIFF_NT": "0",
    "FAM_APPLY_NT": "1",
}

_CHILD = """
import sys
sys.path[:0] = [%r, %r]
import kernel_models as km
from faabric_amd import _core

_core.set_log_level("error")
for n_pages in (33, 2049, 4097):
    km.check_snapshot_geometry(n_pages)
src_dev, src_host = km.random_source(1025 * 16 + 64)
for n_vec in (256, 257, 511, 512, 513, 768, 769, 1025):
    for src_off, dst_off in km.COPY_OFFSETS:
        km.check_copy_buffer(n_vec * 16, src_off, dst_off, src_dev, src_host)
assert (km.to_host(src_dev) == src_host).all()
print("KERNEL_TUNABLES_OK")
"""


@requires_gpu
def test_tunable_paths_in_child_process():
    """The FAM_* variables are read once per process, so a fresh child reruns
    the geometry and copy checks with capped grids (grid-stride loops; at
    copy grid 1 the vector counts cross into and out of the 2-way unrolled
    loop and its tail), cached diff loads and streaming apply."""
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    repo_root = os.path.dirname(tests_dir)
    code = _CHILD % (repo_root, tests_dir)
    r = subprocess.run([sys.executable, "-c", code],
                       env=dict(os.environ, **TUNABLES),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "KERNEL_TUNABLES_OK" in r.stdout
