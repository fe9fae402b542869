"""Numpy models of the MPI collectives in cpp/src/mpi.cpp.

Each model takes the list of per-rank inputs and returns the list of per-rank
expected outputs (None where a rank receives nothing). The element operation
is kernel_models.elementwise_model, which tests/test_kernel_models pins to the
host plane's op_reduce bit for bit; the fold orders are the ones both planes
use:

  reduce         acc = x[root]; for i = 0..size-1, i != root: acc = op(acc, x[i])
  allReduce      reduce at 0, then copy
  scan           acc[r] = op(x[r], acc[r-1]): the rank's own value on the left
  reduceScatter  reduce the full buffer at 0, then slice r
  the rest       pure data movement

The inputs are a deterministic function of (case, rank, index), so every rank
can rebuild every rank's input. They are position dependent: a slice at the
wrong offset, a chunk in the wrong slot or a truncated message shows.

tests/test_mpi_models.py pins these models to the host plane on the CPU;
tests/test_gpu_mpi_device_plane.py holds the device plane to them.
"""

import functools
import itertools

import numpy as np

import kernel_models as km

MPI_OPS = (km.OP_SUM, km.OP_MAX, km.OP_MIN, km.OP_PROD)
DTYPES = tuple(sorted(km.NP_DTYPE))
DTYPE_OP_PAIRS = tuple((d, o) for d in DTYPES for o in MPI_OPS)

_MASK64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


# ---------------------------------------------------------------------------
# Folds
# ---------------------------------------------------------------------------


def reduce_order(size, root):
    """The ranks in the order reduce folds them."""
    return [root] + [i for i in range(size) if i != root]


def reduce_fold(dtype, op, xs, root=0):
    order = reduce_order(len(xs), root)
    acc = np.array(xs[order[0]], dtype=km.NP_DTYPE[dtype])
    for i in order[1:]:
        acc = km.elementwise_model(op, dtype, acc, xs[i])
    return acc


def reduce_model(dtype, op, xs, root):
    """Only the root receives."""
    out = [None] * len(xs)
    out[root] = reduce_fold(dtype, op, xs, root)
    return out


def allreduce_model(dtype, op, xs):
    acc = reduce_fold(dtype, op, xs, 0)
    return [acc] * len(xs)


def scan_model(dtype, op, xs):
    out = [np.array(xs[0], dtype=km.NP_DTYPE[dtype])]
    for r in range(1, len(xs)):
        out.append(km.elementwise_model(op, dtype, xs[r], out[r - 1]))
    return out


def reducescatter_model(dtype, op, xs, recv_count):
    """xs[r] has recv_count * size elements."""
    full = reduce_fold(dtype, op, xs, 0)
    return [full[r * recv_count:(r + 1) * recv_count] for r in range(len(xs))]


def broadcast_model(xs, root):
    return [xs[root]] * len(xs)


def scatter_model(xs, root, count):
    """xs[root] has count * size elements; the other inputs are ignored."""
    return [xs[root][r * count:(r + 1) * count] for r in range(len(xs))]


def gather_model(xs, root):
    out = [None] * len(xs)
    out[root] = np.concatenate(xs)
    return out


def allgather_model(xs):
    full = np.concatenate(xs)
    return [full] * len(xs)


def alltoall_model(xs, count):
    """xs[r] has count * size elements: chunk j of rank r goes to slot r of
    rank j."""
    size = len(xs)
    return [
        np.concatenate([xs[i][r * count:(r + 1) * count] for i in range(size)])
        for r in range(size)
    ]


# ---------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------


def _fold_order_rows(dtype, size):
    """Float tuples on which the fold order shows: with big + 1 == big in the
    dtype, (big, 1, -big, 3) sums to 3 ascending and to 1 descending; the
    product of (huge, huge, 1/huge, 0.5) overflows or not by its order."""
    if not km.is_float(dtype):
        return []
    ft = km.NP_DTYPE[dtype]
    big, huge = (1e8, 1e30) if dtype == km.DT_FLOAT else (1e17, 1e300)
    with np.errstate(over="ignore"):
        assert ft.type(big) + ft.type(3.0) == ft.type(big)
        assert np.isinf(ft.type(huge) * ft.type(huge))
    rows = []
    for base in ([big, 1.0, -big, 3.0], [huge, huge, 1.0 / huge, 0.5]):
        rows += [p[:size] for p in itertools.permutations(base)]
    return rows


def _fits(dtype, op, row):
    """Whether every partial result of every fold the planes run over this
    tuple fits a signed dtype (overflow is undefined on both planes)."""
    ii = np.iinfo(km.NP_DTYPE[dtype])
    for root in range(len(row)):
        order = reduce_order(len(row), root)
        acc = int(row[order[0]])
        for i in order[1:]:
            acc = acc + int(row[i]) if op == km.OP_SUM else acc * int(row[i])
            if acc < ii.min or acc > ii.max:
                return False
    return True


@functools.lru_cache(maxsize=None)
def tuple_table(dtype, op, size):
    """[T, size]: row t holds what the `size` ranks contribute to one element.
    The adversarial values of the dtype against two families of strides, so
    every ordered pairing of rank 0 with rank 1 occurs, plus the fold-order
    rows. For signed integers under SUM/PROD the rows with an overflowing
    partial result are left out, as kernel_models.operand_pairs does."""
    vals = km.adversarial_values(dtype)
    k = len(vals)
    rows = _fold_order_rows(dtype, size)
    for a in range(k):
        for b in range(k):
            rows.append([vals[(a + r * b) % k] for r in range(size)])
            rows.append([vals[(a + b * (r * r + 1) + r) % k]
                         for r in range(size)])
    if dtype in (km.DT_INT32, km.DT_INT64) and op in (km.OP_SUM, km.OP_PROD):
        rows = [row for row in rows if _fits(dtype, op, row)]
    assert rows
    table = np.array(rows, dtype=km.NP_DTYPE[dtype]).reshape(len(rows), size)
    table.setflags(write=False)
    return table


def _hash(n, salt):
    """n well-mixed 64-bit words that depend on index and salt."""
    j = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (j + np.uint64((salt * 7919 + 1) & _MASK64)) * np.uint64(_GOLDEN)
    return km.xorshift64(x)


def reduce_inputs(dtype, op, size, n, salt=0):
    """The inputs of all ranks to a reducing collective of n elements: element
    j is row idx[j] of tuple_table. The first T elements walk the whole table
    once (from a start that depends on salt), the rest pick rows by hash."""
    table = tuple_table(dtype, op, size)
    t = table.shape[0]
    idx = (_hash(n, salt) >> np.uint64(20)) % np.uint64(t)
    head = min(n, t)
    idx[:head] = (np.arange(head, dtype=np.uint64)
                  + np.uint64(salt * 37)) % np.uint64(t)
    picked = table[idx.astype(np.int64)]
    return [np.ascontiguousarray(picked[:, r]) for r in range(size)]


def mover_input(dtype, rank, n, salt=0):
    """One rank's input to a data-moving collective: arbitrary bit patterns
    (data movement must keep every one, NaN payloads included), with an
    adversarial value of the dtype in every fourth element."""
    dt = km.NP_DTYPE[dtype]
    h = _hash(n, salt * 64 + rank + 1)
    ut = np.dtype("u%d" % dt.itemsize)
    out = (h >> np.uint64(64 - 8 * dt.itemsize)).astype(ut).view(dt).copy()
    vals = km.adversarial_values(dtype)
    pick = ((h >> np.uint64(8)) % np.uint64(len(vals))).astype(np.int64)
    out[::4] = vals[pick[::4]]
    return out


def mover_inputs(dtype, size, n, salt=0):
    return [mover_input(dtype, r, n, salt) for r in range(size)]


# ---------------------------------------------------------------------------
# Comparison
# ---------------------------------------------------------------------------


def first_mismatch(dtype, op, got, want):
    """None if `got` equals `want` bit for bit, else (index, got bits, want
    bits) of the first element that differs. One exception, the one
    kernel_models.assert_elementwise_equal makes: where float SUM/PROD gives
    NaN in the model, IEEE 754 leaves payload and sign open (x86 and the GPU
    choose differently), so there `got` only has to be NaN as well. op is
    None for data movement, which has no exception."""
    got = np.asarray(got)
    want = np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return (-1, str((got.dtype, got.shape)), str((want.dtype, want.shape)))
    gb, wb = km.bits(got), km.bits(want)
    differ = gb != wb
    if op is not None and km.is_float(dtype) and op in km.ARITH_OPS:
        differ &= ~(np.isnan(want) & np.isnan(got))
    bad = np.nonzero(differ)[0]
    if bad.size == 0:
        return None
    i = int(bad[0])
    return (i, hex(int(gb[i])), hex(int(wb[i])))
