"""CPU reference models of the typed merge regions of the device snapshot
engine: the typed diff (typedDiffKernel), the TypedElems wire form, the typed
apply (applyTypedElemsKernel) and DeviceSnapshot.diff_with_regions.

Plain numpy, no GPU library and no import of the package; the codes below are
the values of SnapshotDataType and SnapshotMergeOperation.
tests/test_typed_merge_models.py pins the models to the host snapshot engine.
"""

import struct

import numpy as np

import kernel_models as km

PAGE = km.PAGE

# SnapshotDataType
T_RAW, T_BOOL, T_INT, T_LONG, T_FLOAT, T_DOUBLE = range(6)
# SnapshotMergeOperation
(M_BYTEWISE, M_SUM, M_PRODUCT, M_SUBTRACT, M_MAX, M_MIN, M_XOR, M_XOR_PAGES,
 M_TYPED_ELEMS) = range(9)

TYPED_DTYPES = (T_INT, T_LONG, T_FLOAT, T_DOUBLE)
TYPED_OPS = (M_SUM, M_SUBTRACT, M_PRODUCT, M_MAX, M_MIN)

NP_DTYPE = {
    T_INT: np.dtype("<i4"),
    T_LONG: np.dtype("<i8"),
    T_FLOAT: np.dtype("<f4"),
    T_DOUBLE: np.dtype("<f8"),
}
DTYPE_NAME = {T_INT: "int", T_LONG: "long", T_FLOAT: "float",
              T_DOUBLE: "double"}
OP_NAME = {M_SUM: "sum", M_SUBTRACT: "subtract", M_PRODUCT: "product",
           M_MAX: "max", M_MIN: "min"}

# The same element type / operation in kernel_models' codes
KM_DTYPE = {T_INT: km.DT_INT32, T_LONG: km.DT_INT64, T_FLOAT: km.DT_FLOAT,
            T_DOUBLE: km.DT_DOUBLE}
KM_OP = {M_SUM: km.OP_SUM, M_SUBTRACT: km.OP_SUB, M_PRODUCT: km.OP_PROD,
         M_MAX: km.OP_MAX, M_MIN: km.OP_MIN}

CASES = [(d, o) for d in TYPED_DTYPES for o in TYPED_OPS]


def case_id(case):
    return "%s-%s" % (DTYPE_NAME[case[0]], OP_NAME[case[1]])


def is_float(dtype):
    return dtype in (T_FLOAT, T_DOUBLE)


class ZeroOriginal(Exception):
    """A changed Product element whose original is zero."""


def _unsigned(dt):
    return np.dtype("<u%d" % dt.itemsize)


def _trunc_div(cur, orig, dt):
    """Integer division that truncates toward zero, as C++ does."""
    out = np.empty(cur.size, dtype=dt)
    for i, (c, o) in enumerate(zip(cur.tolist(), orig.tolist())):
        q = abs(c) // abs(o)
        out[i] = -q if (c < 0) != (o < 0) else q
    return out


def typed_diff_model(dtype, op, orig, cur):
    """(idx, val) of the typed diff of `cur` against `orig`: ascending element
    indices of the elements with !(orig == cur), and per element cur - orig
    (Sum), orig - cur (Subtract), cur / orig (Product) or cur (Max, Min).
    Integer Sum and Subtract wrap."""
    dt = NP_DTYPE[dtype]
    orig = np.asarray(orig, dtype=dt)
    cur = np.asarray(cur, dtype=dt)
    assert orig.shape == cur.shape and orig.ndim == 1
    changed = ~(orig == cur)  # NaN: always; +0.0 vs -0.0: never
    idx = np.nonzero(changed)[0].astype(np.uint32)
    o, c = orig[changed], cur[changed]
    with np.errstate(all="ignore"):
        if op == M_SUM or op == M_SUBTRACT:
            a, b = (c, o) if op == M_SUM else (o, c)
            if is_float(dtype):
                val = a - b
            else:
                ut = _unsigned(dt)
                val = (a.view(ut) - b.view(ut)).view(dt)
        elif op == M_PRODUCT:
            if np.any(o == 0):
                raise ZeroOriginal()
            val = c / o if is_float(dtype) else _trunc_div(c, o, dt)
        elif op in (M_MAX, M_MIN):
            val = c.copy()
        else:
            raise ValueError("not a typed merge operation: %r" % op)
    assert val.dtype == dt
    return idx, val


def typed_apply_model(dtype, op, base, idx, val):
    """base[idx[i]] = op(base[idx[i]], val[i]); every index at most once.
    Max and Min are std::max/std::min(target, value): a NaN operand or a
    +0.0/-0.0 tie keeps the target."""
    dt = NP_DTYPE[dtype]
    out = np.array(base, dtype=dt)
    idx = np.asarray(idx, dtype=np.int64)
    assert np.unique(idx).size == idx.size
    out[idx] = km.elementwise_model(
        KM_OP[op], KM_DTYPE[dtype], out[idx], np.asarray(val, dtype=dt))
    return out


# ---------------------------------------------------------------------------
# TypedElems wire form:
#   [u32 op][u32 count][u32 elemIdx[count]][zero pad to 8 B][T value[count]]
# ---------------------------------------------------------------------------


def packed_size(count, itemsize):
    return ((8 + 4 * count + 7) & ~7) + count * itemsize


def pack_typed_elems(dtype, op, idx, val):
    dt = NP_DTYPE[dtype]
    idx = np.asarray(idx, dtype="<u4")
    val = np.asarray(val, dtype=dt)
    assert idx.size == val.size
    head = struct.pack("<II", op, idx.size) + idx.tobytes()
    head += b"\x00" * (-len(head) % 8)
    return head + val.tobytes()


def unpack_typed_elems(dtype, data):
    """(op, idx, val) of a packed diff; checks the size and the padding."""
    dt = NP_DTYPE[dtype]
    op, count = struct.unpack_from("<II", data, 0)
    assert len(data) == packed_size(count, dt.itemsize), (len(data), count)
    idx = np.frombuffer(data, dtype="<u4", count=count, offset=8)
    val_off = len(data) - count * dt.itemsize
    assert data[8 + 4 * count:val_off] == b"\x00" * (val_off - 8 - 4 * count)
    val = np.frombuffer(data, dtype=dt, count=count, offset=val_off)
    return op, idx, val


def sort_entries(idx, val):
    """Entries in ascending index order (the device order is unspecified);
    asserts that no index occurs twice."""
    idx = np.asarray(idx)
    order = np.argsort(idx, kind="stable")
    idx, val = idx[order], np.asarray(val)[order]
    assert np.unique(idx).size == idx.size, "an index occurs twice"
    return idx, val


def assert_values_equal(dtype, op, got, want, what=""):
    """Raw bits, except that a Sum, Subtract or Product value that is NaN in
    the model only has to be NaN (kernel_models.assert_elementwise_equal)."""
    km.assert_elementwise_equal(KM_OP[op], KM_DTYPE[dtype], got, want, what)


# ---------------------------------------------------------------------------
# Regions: (offset, length, dtype, op), length 0 = to the end of the arena
# ---------------------------------------------------------------------------


def region_span(region, arena_size):
    """(offset, end, element count) of a typed region."""
    off, length, dtype, _ = region
    end = arena_size if length == 0 else min(arena_size, off + length)
    return off, end, (end - off) // NP_DTYPE[dtype].itemsize


def is_typed(region):
    return region[3] in TYPED_OPS


def diff_with_regions_model(base, cur, regions):
    """DeviceSnapshot.diff_with_regions on uint8 arrays of a whole arena.

    Returns (typed, pages, payload): typed is a list of (offset, dtype, op,
    idx, val) for the typed regions that changed, in offset order; pages the
    sorted page list of the XorPages diff and payload its rows, one 4 KiB row
    per listed page. The XOR payload is zero over every typed region's bytes,
    and a page that lies wholly inside typed regions is not listed, dirty or
    not."""
    base = np.asarray(base, dtype=np.uint8)
    cur = np.asarray(cur, dtype=np.uint8)
    n = base.size
    assert n % PAGE == 0 and cur.size == n
    typed_regions = sorted(r for r in regions if is_typed(r))
    typed = []
    covered = np.zeros(n, dtype=bool)
    for r in typed_regions:
        off, end, count = region_span(r, n)
        dt = NP_DTYPE[r[2]]
        covered[off:end] = True
        o = base[off:off + count * dt.itemsize].view(dt)
        c = cur[off:off + count * dt.itemsize].view(dt)
        idx, val = typed_diff_model(r[2], r[3], o, c)
        if idx.size:
            typed.append((off, r[2], r[3], idx, val))
    xor = (base ^ cur).reshape(n // PAGE, PAGE)
    dirty = xor.any(1)
    wholly = covered.reshape(n // PAGE, PAGE).all(1)
    xor = np.where(covered.reshape(n // PAGE, PAGE), 0, xor).astype(np.uint8)
    pages = np.nonzero(dirty & ~wholly)[0].tolist()
    return typed, pages, xor[pages]


def apply_region_diffs_model(base, typed, pages, payload):
    """The arena after merging one diff_with_regions result into `base`."""
    out = np.array(base, dtype=np.uint8)
    for off, dtype, op, idx, val in typed:
        dt = NP_DTYPE[dtype]
        last = int(idx.max()) + 1
        view = out[off:off + last * dt.itemsize].view(dt)
        view[:] = typed_apply_model(dtype, op, view, idx, val)
    for row, p in zip(payload, pages):
        out[p * PAGE:(p + 1) * PAGE] ^= row
    return out


# ---------------------------------------------------------------------------
# Operands
# ---------------------------------------------------------------------------


def host_operands(dtype, op):
    """(orig, cur) for the host engine: every ordered pairing of
    kernel_models.operand_pairs (NaN, +-0.0, extrema, wrap). Under Product
    the pairings with a zero original that changed are left out: the host
    diff throws on them (see zero_original_operands)."""
    orig, cur = km.operand_pairs(KM_DTYPE[dtype], KM_OP[op])
    if op == M_PRODUCT:
        keep = ~((orig == 0) & ~(orig == cur))
        orig, cur = orig[keep], cur[keep]
    return orig, cur


def exact_product_operands(dtype, n):
    """(orig, cur): originals are powers of two of either sign and cur is
    orig times a small integer, so cur / orig is exact and so is the product
    back. The multiplier 1 leaves elements unchanged, 0 zeroes them."""
    dt = NP_DTYPE[dtype]
    i = np.arange(n)
    mult = np.array([3, 1, -5, 7, 0, 2, -1, 6])[i % 8]
    sign = np.where(i % 3 == 0, -1, 1)
    if is_float(dtype):
        orig = (sign * np.exp2((i % 21) - 10)).astype(dt)
    else:
        orig = (sign * (1 << (i % 20))).astype(dt)
    cur = (orig * mult.astype(dt)).astype(dt)
    return orig, cur


def device_operands(dtype, op, n):
    """(orig, cur) of n elements for the device diff. Product takes the exact
    operands; the others tile kernel_models.operands, with NaN originals
    replaced by 1.5 so that a pattern decides alone which elements change (a
    NaN original is covered by nan_original_operands)."""
    if op == M_PRODUCT:
        return exact_product_operands(dtype, n)
    orig, cur = km.operands(KM_DTYPE[dtype], KM_OP[op], n)
    if is_float(dtype):
        orig = np.where(np.isnan(orig), orig.dtype.type(1.5), orig)
    return orig, cur


CHANGE_PATTERNS = ("none", "all", "every_third", "first", "last")


def change_positions(pattern, n):
    i = np.arange(n)
    return {
        "none": i[:0],
        "all": i,
        "every_third": i[::3],
        "first": i[:1],
        "last": i[n - 1:],
    }[pattern]


def patterned(orig, cur, pattern):
    """cur's values at the pattern's positions, orig's bits elsewhere."""
    out = orig.copy()
    pos = change_positions(pattern, orig.size)
    out[pos] = cur[pos]
    return out
