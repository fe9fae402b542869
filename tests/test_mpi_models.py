"""The collective models in mpi_models.py against the host plane, bit for
bit, in worlds of 3 and 4 ranks: every (dtype, op) pair through reduce,
allReduce, scan and reduceScatter, every root position, and the data movers.
This anchors the models to a plane that runs without a GPU; the device plane
is held to the same models in tests/test_gpu_mpi_device_plane.py."""

import json

import numpy as np
import pytest

import kernel_models as km
import mpi_models as mm
from faabric_amd import _core
from faabric_amd.runtime import LocalRuntime, wait_for_batch

WORLD_SIZES = (3, 4)
COUNTS = (1, 3, 1027)


def roots(size):
    return sorted({0, size // 2, size - 1})


def host_cases(size):
    """(id, kind, dtype, op, count, root). Every rank walks the same list."""
    cases = []
    for salt, (dtype, op) in enumerate(mm.DTYPE_OP_PAIRS):
        name = "%s-%s" % (km.DTYPE_NAME[dtype], km.OP_NAME[op])
        for n in COUNTS:
            for root in roots(size):
                cases.append(("reduce-%s-n%d-root%d" % (name, n, root),
                              "reduce", dtype, op, n, root, salt))
            for kind in ("allreduce", "scan", "reducescatter"):
                cases.append(("%s-%s-n%d" % (kind, name, n),
                              kind, dtype, op, n, 0, salt))
    for salt, dtype in enumerate(mm.DTYPES):
        name = km.DTYPE_NAME[dtype]
        for n in COUNTS:
            for root in roots(size):
                for kind in ("bcast", "scatter", "gather"):
                    cases.append(("%s-%s-n%d-root%d" % (kind, name, n, root),
                                  kind, dtype, None, n, root, salt))
            for kind in ("allgather", "alltoall"):
                cases.append(("%s-%s-n%d" % (kind, name, n),
                              kind, dtype, None, n, 0, salt))
    return cases


def _run_case(rank, size, case):
    """(got, want) of this rank; want None where the rank receives nothing."""
    _, kind, dtype, op, n, root, salt = case
    dt = km.NP_DTYPE[dtype]
    mdt = _core.MpiDataType(dtype)
    mop = _core.MpiOp(op) if op is not None else None

    def arr(data):
        return np.frombuffer(data, dtype=dt)

    if kind in ("reduce", "allreduce", "scan"):
        xs = mm.reduce_inputs(dtype, op, size, n, salt)
        mine = xs[rank].tobytes()
        if kind == "reduce":
            got = _core.mpi_reduce_bytes(rank, root, mine, mdt, mop)
            return arr(got), mm.reduce_model(dtype, op, xs, root)[rank]
        if kind == "allreduce":
            got = _core.mpi_allreduce_bytes(rank, mine, mdt, mop)
            return arr(got), mm.allreduce_model(dtype, op, xs)[rank]
        got = _core.mpi_scan_bytes(rank, mine, mdt, mop)
        return arr(got), mm.scan_model(dtype, op, xs)[rank]
    if kind == "reducescatter":
        xs = mm.reduce_inputs(dtype, op, size, n * size, salt)
        got = _core.mpi_reducescatter_bytes(rank, xs[rank].tobytes(), mdt, n,
                                            mop)
        return arr(got), mm.reducescatter_model(dtype, op, xs, n)[rank]

    nbytes = n * dt.itemsize
    if kind == "bcast":
        xs = mm.mover_inputs(dtype, size, n, salt)
        data = xs[rank].tobytes() if rank == root else b""
        got = _core.mpi_bcast_bytes(root, rank, data, nbytes)
        return arr(got), mm.broadcast_model(xs, root)[rank]
    if kind == "scatter":
        xs = mm.mover_inputs(dtype, size, n * size, salt)
        data = xs[rank].tobytes() if rank == root else b""
        got = _core.mpi_scatter_bytes(root, rank, data, nbytes)
        return arr(got), mm.scatter_model(xs, root, n)[rank]
    if kind == "gather":
        xs = mm.mover_inputs(dtype, size, n, salt)
        got = _core.mpi_gather_bytes(rank, root, xs[rank].tobytes(), size)
        return arr(got), mm.gather_model(xs, root)[rank]
    if kind == "allgather":
        xs = mm.mover_inputs(dtype, size, n, salt)
        got = _core.mpi_allgather_bytes(rank, xs[rank].tobytes(), size)
        return arr(got), mm.allgather_model(xs)[rank]
    assert kind == "alltoall"
    xs = mm.mover_inputs(dtype, size, n * size, salt)
    got = _core.mpi_alltoall_bytes(rank, xs[rank].tobytes(), size)
    return arr(got), mm.alltoall_model(xs, n)[rank]


def _model_payload(msg):
    _, rank, size = _core.mpi_init()
    bad = []
    for case in host_cases(size):
        got, want = _run_case(rank, size, case)
        if want is None:
            continue
        miss = mm.first_mismatch(case[2], case[3], got, want)
        if miss is not None:
            bad.append([case[0], rank, *miss])
    _core.mpi_barrier(rank)
    msg.output_data = json.dumps(bad[:20])
    return 1 if bad else 0


@pytest.fixture(scope="module")
def results():
    """Both worlds run once; the tests assert on what the ranks recorded."""
    rt = LocalRuntime(slots=max(WORLD_SIZES))
    rt.start_planner(with_snapshot_server=False)
    rt.start_worker()
    out = {}
    try:
        _core.register_function("mpimodel", "hostplane", _model_payload)
        for size in WORLD_SIZES:
            ber = _core.batch_exec_factory("mpimodel", "hostplane", 1)
            msgs = ber.messages
            msgs[0].is_mpi = True
            msgs[0].mpi_world_size = size
            ber.messages = msgs
            decision = _core.call_functions(ber)
            assert decision.app_id == ber.app_id, decision.app_id
            out[size] = wait_for_batch(ber.app_id, size, 120_000)
    finally:
        rt.stop()
    return out


@pytest.mark.parametrize("size", WORLD_SIZES)
def test_host_plane_equals_models(results, size):
    res = results[size]
    assert sorted(r.mpi_rank for r in res) == list(range(size))
    for r in res:
        assert r.return_value == 0, (r.mpi_rank, r.output_data)
        assert json.loads(r.output_data) == []


def test_case_table_covers_the_issue():
    for size in WORLD_SIZES:
        cases = host_cases(size)
        assert len({c[0] for c in cases}) == len(cases)
        assert roots(size) == [0, size // 2, size - 1]
        for kind in ("reduce", "allreduce", "scan", "reducescatter"):
            seen = {(c[2], c[3], c[4]) for c in cases if c[1] == kind}
            assert seen == {(d, o, n) for d, o in mm.DTYPE_OP_PAIRS
                            for n in COUNTS}
        for kind in ("reduce", "bcast", "scatter", "gather"):
            assert {c[5] for c in cases if c[1] == kind} == set(roots(size))
        assert {c[1] for c in cases} >= {"allgather", "alltoall"}


def test_models_by_hand():
    """The fold orders, on values worked out by hand."""
    f = km.DT_FLOAT
    xs = [np.array([v], dtype=np.float32) for v in (1e8, 1.0, -1e8, 3.0)]
    # root 0: ((1e8 + 1) - 1e8) + 3; root 2: ((-1e8 + 1e8) + 1) + 3
    assert mm.reduce_fold(f, km.OP_SUM, xs, 0).tolist() == [3.0]
    assert mm.reduce_fold(f, km.OP_SUM, xs, 2).tolist() == [4.0]
    assert mm.reduce_order(4, 2) == [2, 0, 1, 3]
    # scan keeps the rank's own value on the left: ties keep it
    zs = [np.array([v], dtype=np.float32) for v in (0.0, -0.0)]
    got = mm.scan_model(f, km.OP_MAX, zs)
    assert np.signbit(got[1][0]) and not np.signbit(got[0][0])
    nan = np.float32("nan")
    got = mm.scan_model(f, km.OP_MAX, [np.array([nan], np.float32),
                                       np.array([1.0], np.float32)])
    assert got[1].tolist() == [1.0]  # op(1.0, nan) keeps the left operand
    got = mm.reduce_fold(f, km.OP_MAX, [np.array([nan], np.float32),
                                        np.array([1.0], np.float32)], 0)
    assert np.isnan(got[0])
    # data movement
    a = [np.arange(4, dtype=np.int32) + 10 * r for r in range(2)]
    assert [x.tolist() for x in mm.alltoall_model(a, 2)] == [
        [0, 1, 10, 11], [2, 3, 12, 13]]
    assert [x.tolist() for x in mm.scatter_model(a, 1, 2)] == [
        [10, 11], [12, 13]]
    assert mm.gather_model(a, 1)[0] is None
    assert mm.gather_model(a, 1)[1].tolist() == [0, 1, 2, 3, 10, 11, 12, 13]
    rs = mm.reducescatter_model(km.DT_INT32, km.OP_SUM, a, 2)
    assert [x.tolist() for x in rs] == [[10, 12], [14, 16]]


def test_inputs_are_position_dependent_and_in_range():
    for dtype, op in mm.DTYPE_OP_PAIRS:
        for size in (2, 3, 4):
            table = mm.tuple_table(dtype, op, size)
            xs = mm.reduce_inputs(dtype, op, size, 1027, 5)
            assert table.shape[0] <= 1027  # count 1027 walks every row
            rows = {tuple(km.bits(r).tolist()) for r in table}
            seen = {tuple(int(km.bits(x)[j]) for x in xs)
                    for j in range(1027)}
            assert seen == rows
            # no run of one value: a shifted slice cannot look the same
            assert not np.array_equal(km.bits(xs[0][:-1]), km.bits(xs[0][1:]))
            if dtype in (km.DT_INT32, km.DT_INT64) and op in (km.OP_SUM,
                                                              km.OP_PROD):
                ii = np.iinfo(km.NP_DTYPE[dtype])
                exact = [sum(int(v) for v in r) if op == km.OP_SUM
                         else int(np.prod([int(v) for v in r], dtype=object))
                         for r in table]
                assert all(ii.min <= e <= ii.max for e in exact)
    for dtype in mm.DTYPES:
        a = mm.mover_input(dtype, 0, 1027, 1)
        b = mm.mover_input(dtype, 1, 1027, 1)
        c = mm.mover_input(dtype, 0, 1027, 2)
        assert not np.array_equal(km.bits(a), km.bits(b))
        assert not np.array_equal(km.bits(a), km.bits(c))
        assert np.array_equal(km.bits(a), km.bits(
            mm.mover_input(dtype, 0, 1027, 1)))


def test_fold_order_rows_tell_orders_apart():
    """The rows that make a descending fold visible do so in the model."""
    for dtype in (km.DT_FLOAT, km.DT_DOUBLE):
        for size in (3, 4):
            xs = mm.reduce_inputs(dtype, km.OP_SUM, size, 1027, 0)
            asc = mm.reduce_fold(dtype, km.OP_SUM, xs, 0)
            acc = xs[0]
            for i in range(size - 1, 0, -1):
                acc = km.elementwise_model(km.OP_SUM, dtype, acc, xs[i])
            assert mm.first_mismatch(dtype, km.OP_SUM, acc, asc) is not None
