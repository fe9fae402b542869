"""CPU reference models of the kernels in cpp/hip/snapshot_kernels.hip, and
the device checks built on them.

The models are plain numpy and import no GPU library; tests/test_kernel_models
pins them to the host plane on the CPU. The check_* functions drive the
device kernels and compare the raw bits with the models; they are shared by
tests/test_gpu_kernels.py and the child process it starts to run the tunable
paths (the FAM_* variables are read once per process).
"""

import numpy as np

PAGE = 4096

# MpiDataType / famElementwiseOp dtype codes
DT_INT32, DT_INT64, DT_UINT64, DT_FLOAT, DT_DOUBLE, DT_BYTE = range(6)
# FamOp codes (0..3 are MpiOp as well)
OP_SUM, OP_MAX, OP_MIN, OP_PROD, OP_SUB, OP_XOR = range(6)

NP_DTYPE = {
    DT_INT32: np.dtype("<i4"),
    DT_INT64: np.dtype("<i8"),
    DT_UINT64: np.dtype("<u8"),
    DT_FLOAT: np.dtype("<f4"),
    DT_DOUBLE: np.dtype("<f8"),
    DT_BYTE: np.dtype("u1"),
}
DTYPE_NAME = {
    DT_INT32: "int32", DT_INT64: "int64", DT_UINT64: "uint64",
    DT_FLOAT: "float", DT_DOUBLE: "double", DT_BYTE: "byte",
}
OP_NAME = {
    OP_SUM: "sum", OP_MAX: "max", OP_MIN: "min", OP_PROD: "prod",
    OP_SUB: "sub", OP_XOR: "xor",
}
ARITH_OPS = (OP_SUM, OP_PROD, OP_SUB)


def is_float(dtype):
    return dtype in (DT_FLOAT, DT_DOUBLE)


def bits(a):
    """The raw bits of an array as unsigned integers of the same width."""
    a = np.ascontiguousarray(a)
    return a.view(np.dtype("u%d" % a.dtype.itemsize))


# ---------------------------------------------------------------------------
# Elementwise op: inout[i] = op(inout[i], in[i]), host-plane semantics
# ---------------------------------------------------------------------------


def elementwise_model(op, dtype, inout, inp):
    """std::max/std::min(inout, in) operand order for MAX/MIN; SUM, SUB and
    PROD in the dtype's own width (one IEEE operation is correctly rounded,
    unsigned types wrap); XOR for bytes only."""
    dt = NP_DTYPE[dtype]
    inout = np.asarray(inout, dtype=dt)
    inp = np.asarray(inp, dtype=dt)
    with np.errstate(all="ignore"):
        if op == OP_SUM:
            out = inout + inp
        elif op == OP_SUB:
            out = inout - inp
        elif op == OP_PROD:
            out = inout * inp
        elif op == OP_MAX:
            out = np.where(inout < inp, inp, inout)
        elif op == OP_MIN:
            out = np.where(inp < inout, inp, inout)
        elif op == OP_XOR and dtype == DT_BYTE:
            out = inout ^ inp
        else:
            raise ValueError("no such (dtype, op): %r %r" % (dtype, op))
    assert out.dtype == dt
    return out


def _float_values(dtype):
    ft = NP_DTYPE[dtype]
    fi = np.finfo(ft)
    ut = np.dtype("u%d" % ft.itemsize)
    mant = fi.nmant
    quiet_nan = ((1 << (fi.nexp + 1)) - 1) << (mant - 1)  # 0x7fc00000
    from_bits = [
        quiet_nan,
        1,                       # smallest subnormal
        (1 << mant) - 1,         # largest subnormal
        (1 << (ft.itemsize * 8 - 1)) | ((1 << mant) - 1),  # its negative
    ]
    special = np.array(from_bits, dtype=ut).view(ft)
    plain = np.array(
        [0.0, -0.0, np.inf, -np.inf, fi.tiny, fi.max, -fi.max, 1.0,
         np.nextafter(ft.type(1.0), ft.type(2.0)), 3.5, -2.25, 1e-3],
        dtype=ft,
    )
    return np.concatenate([plain, special])


def adversarial_values(dtype):
    """The fixed value set of a dtype (special values first)."""
    if is_float(dtype):
        return _float_values(dtype)
    dt = NP_DTYPE[dtype]
    if dtype in (DT_INT32, DT_INT64):
        ii = np.iinfo(dt)
        return np.array(
            [ii.min, ii.max, -1, 0, 1, ii.min + 1, ii.max - 1, 2, -3, 1000,
             -46341, 46340],
            dtype=dt,
        )
    if dtype == DT_UINT64:
        return np.array(
            [0, 1, 2**63 - 1, 2**63, 2**63 + 5, 2**64 - 1, 3, 0x9E3779B97F4A7C15],
            dtype=dt,
        )
    return np.array([0, 1, 100, 127, 128, 200, 255], dtype=dt)


def _signed_overflows(op, a, b, ii):
    r = {OP_SUM: a + b, OP_SUB: a - b, OP_PROD: a * b}[op]
    return r < ii.min or r > ii.max


def operand_pairs(dtype, op):
    """(inout, in): the value set against every rotation of itself, so each
    ordered pairing occurs once. For signed integers under SUM/SUB/PROD the
    pairings whose exact result overflows are left out (undefined on both
    planes)."""
    vals = adversarial_values(dtype)
    k = len(vals)
    left = np.tile(vals, k)
    right = np.concatenate([np.roll(vals, -r) for r in range(k)])
    if dtype in (DT_INT32, DT_INT64) and op in ARITH_OPS:
        ii = np.iinfo(NP_DTYPE[dtype])
        keep = np.array(
            [not _signed_overflows(op, int(a), int(b), ii)
             for a, b in zip(left, right)]
        )
        left, right = left[keep], right[keep]
    return left, right


def operands(dtype, op, n):
    """n elements of each operand, tiled from operand_pairs."""
    left, right = operand_pairs(dtype, op)
    return np.resize(left, n), np.resize(right, n)


def assert_elementwise_equal(op, dtype, got, want, what=""):
    """Bit-for-bit, except that where SUM/SUB/PROD give NaN in the model the
    device result only has to be NaN too (payload and sign differ between
    x86 and the GPU)."""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gb, wb = bits(got), bits(want)
    if is_float(dtype) and op in ARITH_OPS:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (
            "%s: NaN positions differ at %s"
            % (what, np.nonzero(np.isnan(got) != nan)[0][:8]))
        gb, wb = gb[~nan], wb[~nan]
    bad = np.nonzero(gb != wb)[0]
    assert bad.size == 0, "%s: %d mismatches, first at %d: got %#x want %#x" % (
        what, bad.size, bad[0], int(gb[bad[0]]), int(wb[bad[0]]))


# ---------------------------------------------------------------------------
# Bench-input kernels
# ---------------------------------------------------------------------------

_U64 = np.uint64
_GOLDEN = _U64(0x9E3779B97F4A7C15)


def xorshift64(x):
    x = np.array(x, dtype=np.uint64)
    x = x ^ (x << _U64(13))
    x = x ^ (x >> _U64(7))
    x = x ^ (x << _U64(17))
    return x


def fill_random_model(n_words, seed):
    """Words written by fillRandomKernel."""
    i = np.arange(n_words, dtype=np.uint64)
    return xorshift64(_U64(seed) ^ (i * _GOLDEN) ^ (i >> _U64(3)))


def touch_pages_model(words, pages, seed):
    """touchPagesKernel on a buffer of uint64 words: every word of each listed
    (distinct) page is XORed with xorshift64(seed ^ word index)."""
    out = np.array(words, dtype=np.uint64)
    per_page = PAGE // 8
    for p in pages:
        idx = np.arange(p * per_page, (p + 1) * per_page, dtype=np.uint64)
        out[p * per_page:(p + 1) * per_page] ^= xorshift64(_U64(seed) ^ idx)
    return out


# ---------------------------------------------------------------------------
# Page diff
# ---------------------------------------------------------------------------


def dirty_flags_model(base, upd):
    n_pages = base.size // PAGE
    return (base != upd).reshape(n_pages, PAGE).any(1)


def dirty_set_model(base, upd):
    return np.nonzero(dirty_flags_model(base, upd))[0].tolist()


def payload_model(base, upd):
    """XOR payload of the whole region, one row per page."""
    return (base ^ upd).reshape(base.size // PAGE, PAGE)


def dirty_patterns(n_pages):
    """name -> sorted dirty page list, for the patterns that exist at this
    page count."""
    pats = {
        "none": [],
        "all": list(range(n_pages)),
        "first": [0],
        "last": [n_pages - 1],
        "every_other": list(range(0, n_pages, 2)),
    }
    if n_pages > 32:
        pats["31_32"] = [31, 32]
    if n_pages > 2048:
        pats["2047_2048"] = [2047, 2048]
    return pats


def flip_pages(base, pages):
    """A copy of base in which each listed page differs in one bit, at a byte
    offset that moves through the whole page with the page number."""
    upd = base.copy()
    for p in pages:
        off = (p * 1021 + 7) % PAGE
        upd[p * PAGE + off] ^= np.uint8(1 << (p % 8))
    return upd


# ---------------------------------------------------------------------------
# Device checks (need torch with a GPU and the built module)
# ---------------------------------------------------------------------------


def to_device(arr):
    import torch

    host = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    return torch.from_numpy(host.copy()).to("cuda")


def to_host(t):
    return t.cpu().numpy()


def check_diff(snap, base, upd, what=""):
    """One full diff of device snapshot `snap` (holding `base`) against `upd`:
    flags, count, index list, payload, apply, and an empty second diff."""
    import torch

    n_pages = base.size // PAGE
    want = dirty_set_model(base, upd)
    want_payload = payload_model(base, upd)
    dev = to_device(upd)
    torch.cuda.synchronize()

    flags = snap.dirty_pages(dev.data_ptr())
    assert len(flags) == n_pages, what
    assert [i for i, f in enumerate(flags) if f] == want, what

    assert snap.diff_xor(dev.data_ptr()) == len(want), what
    pages, payload = snap.gather_last_diff()
    assert len(pages) == len(want), what
    assert sorted(pages) == want, what  # equal lengths: no duplicates
    got = np.frombuffer(payload, dtype=np.uint8).reshape(len(pages), PAGE)
    assert np.array_equal(
        got, want_payload[np.asarray(pages, dtype=np.int64)]), what

    snap.apply_last_diff()
    out = np.frombuffer(snap.copy_out_host(base.size), dtype=np.uint8)
    assert np.array_equal(out, upd), what
    assert snap.diff_xor(dev.data_ptr()) == 0, what
    pages, payload = snap.gather_last_diff()
    assert list(pages) == [] and payload == b"", what


def check_snapshot_geometry(n_pages, seed=0):
    """Every dirty pattern at one page count, each from a fresh capture."""
    import torch
    from faabric_amd import _core

    rng = np.random.default_rng(1000 + seed + n_pages)
    base = rng.integers(0, 256, n_pages * PAGE, dtype=np.uint8)
    base_dev = to_device(base)
    torch.cuda.synchronize()
    snap = _core.DeviceSnapshot(n_pages * PAGE)
    for name, pages in dirty_patterns(n_pages).items():
        snap.capture_from_ptr(base_dev.data_ptr())
        check_diff(snap, base, flip_pages(base, pages),
                   "%d pages, %s" % (n_pages, name))


COPY_OFFSETS = [(0, 0), (4, 0), (0, 4), (4, 4), (1, 0), (0, 1), (1, 1)]
COPY_GUARD = 64


def check_copy_buffer(nbytes, src_off, dst_off, src_dev, src_host):
    """fam_copy_buffer of nbytes from src_dev+src_off into the middle of a
    guarded destination at a pointer offset of dst_off from 16 B alignment."""
    import torch
    from faabric_amd import _core

    assert src_off + nbytes <= src_host.size
    lead = COPY_GUARD + dst_off  # COPY_GUARD keeps the 16 B alignment
    total = lead + nbytes + COPY_GUARD
    guard = (np.arange(total, dtype=np.uint32) * 7 + 3).astype(np.uint8)
    dst = to_device(guard)
    assert dst.data_ptr() % 16 == 0 and src_dev.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    _core.fam_copy_buffer(src_dev.data_ptr() + src_off,
                          dst.data_ptr() + lead, nbytes)
    want = guard.copy()
    want[lead:lead + nbytes] = src_host[src_off:src_off + nbytes]
    got = to_host(dst)
    assert np.array_equal(got, want), (
        "copy %d B src+%d dst+%d" % (nbytes, src_off, dst_off))


def random_source(nbytes, seed=7):
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, nbytes, dtype=np.uint8)
    return to_device(host), host
