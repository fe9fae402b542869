"""The MPI device plane (PTP / HIP-IPC, the only multi-rank device path on
one GPU) against the numpy models in mpi_models.py, bit for bit.

Two launch arrangements, each started once per module:

  in-process     one child process with 3 slots runs worlds of 1, 2 and 3
                 ranks, each through the whole case table
  cross-process  two worker processes with one slot each run the table at
                 world size 2, so the HIP-IPC arena path sees the same data

Every rank rebuilds all ranks' inputs, works out its own expected output with
the model, copies its device buffers back and compares bits; it hands the
mismatches back as JSON in the message output. The tests below only assert on
what those launches recorded. FAABRIC_DEVICE_PLANE is read once per process,
so the children set it before they import the package.
"""

import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np
import pytest

import kernel_models as km
import mpi_models as mm

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

GUARD = 64  # bytes on both sides of every buffer; keeps 16 B alignment
INPROC_OFFSET = 15500
CROSS_BASE = 16100
CROSS_STEP = 300
INPROC_SIZES = (1, 2, 3)
CROSS_SIZE = 2
REDUCERS = ("reduce", "allreduce", "scan", "reducescatter")
MOVERS = ("sendrecv_ring", "send_recv", "isend_irecv", "bcast", "allgather",
          "alltoall", "scatter", "gather")


# ---------------------------------------------------------------------------
# Case table
# ---------------------------------------------------------------------------


def roots(size):
    return sorted({0, size // 2, size - 1})


def _case(kind, dtype, op, n, root=0, inplace=False, send_off=0, recv_off=0,
          salt=0):
    name = "%s-%s" % (kind, km.DTYPE_NAME[dtype])
    if op is not None:
        name += "-" + km.OP_NAME[op]
    name += "-n%d" % n
    if root:
        name += "-root%d" % root
    if inplace:
        name += "-inplace"
    if send_off or recv_off:
        name += "-off%d_%d" % (send_off, recv_off)
    return dict(id=name, kind=kind, dtype=dtype, op=op, n=n, root=root,
                inplace=inplace, send_off=send_off, recv_off=recv_off,
                salt=salt)


def device_cases(size):
    """The smallest shapes that reach each branch. 1027 elements of 4 or 8
    bytes are no multiple of 16 B, so every chunk i >= 1 of a chunked buffer
    starts 4 B- or 8 B-aligned only and famCopyBuffer takes its
    non-vectorised branch; 4099 does the same for bytes."""
    cases = []
    main_n = {km.DT_BYTE: 4099}
    # every (dtype, op) through the four reducing collectives
    for salt, (dtype, op) in enumerate(mm.DTYPE_OP_PAIRS):
        for kind in REDUCERS:
            cases.append(_case(kind, dtype, op, main_n.get(dtype, 1027),
                               salt=salt))
    # every dtype through the data movers
    for salt, dtype in enumerate(mm.DTYPES):
        for kind in MOVERS:
            cases.append(_case(kind, dtype, None, main_n.get(dtype, 1027),
                               salt=salt))
    # counts
    for n in (0, 1, 257, 65537):
        for kind in REDUCERS:
            cases.append(_case(kind, km.DT_FLOAT, km.OP_SUM, n, salt=n))
            cases.append(_case(kind, km.DT_INT64, km.OP_MAX, n, salt=n))
        for kind in MOVERS:
            cases.append(_case(kind, km.DT_FLOAT, None, n, salt=n))
        cases.append(_case("alltoall", km.DT_BYTE, None, n, salt=n))
    # roots
    for root in roots(size)[1:]:
        for dtype, op in ((km.DT_FLOAT, km.OP_SUM), (km.DT_DOUBLE, km.OP_MAX),
                          (km.DT_BYTE, km.OP_PROD)):
            cases.append(_case("reduce", dtype, op, main_n.get(dtype, 1027),
                               root=root, salt=40 + root))
        for kind in ("bcast", "scatter", "gather"):
            for dtype in (km.DT_FLOAT, km.DT_BYTE, km.DT_UINT64):
                cases.append(_case(kind, dtype, None,
                                   main_n.get(dtype, 1027), root=root,
                                   salt=50 + root))
    # in place
    for kind in ("reduce", "allreduce", "scan"):
        for dtype, op in ((km.DT_FLOAT, km.OP_SUM), (km.DT_UINT64, km.OP_MIN)):
            for root in (roots(size) if kind == "reduce" else [0]):
                cases.append(_case(kind, dtype, op, 1027, root=root,
                                   inplace=True, salt=60))
    for dtype in (km.DT_FLOAT, km.DT_BYTE):
        cases.append(_case("allgather", dtype, None, main_n.get(dtype, 1027),
                           inplace=True, salt=61))
    # base pointers at a 4 B offset from 16 B alignment
    for send_off, recv_off in ((4, 0), (0, 4), (4, 4)):
        for kind in REDUCERS:
            cases.append(_case(kind, km.DT_FLOAT, km.OP_SUM, 1027,
                               root=roots(size)[-1] if kind == "reduce" else 0,
                               send_off=send_off, recv_off=recv_off, salt=70))
        for kind in MOVERS:
            cases.append(_case(kind, km.DT_FLOAT, None, 1027,
                               root=roots(size)[-1],
                               send_off=send_off, recv_off=recv_off, salt=71))
        # a multiple of 16 B, so only the base pointer decides the branch
        cases.append(_case("allreduce", km.DT_FLOAT, km.OP_SUM, 1024,
                           send_off=send_off, recv_off=recv_off, salt=72))
        cases.append(_case("alltoall", km.DT_FLOAT, None, 1024,
                           send_off=send_off, recv_off=recv_off, salt=72))
    # MPI matching order on one channel
    for n in (1027, 1):
        cases.append(_case("order_irecv_recv", km.DT_FLOAT, None, n, salt=80))
        cases.append(_case("order_irecv_irecv", km.DT_FLOAT, None, n,
                           salt=81))
    # one host and one device buffer in sendRecv
    for kind in ("sendrecv_host_to_dev", "sendrecv_dev_to_host"):
        for dtype in (km.DT_FLOAT, km.DT_BYTE):
            cases.append(_case(kind, dtype, None, main_n.get(dtype, 1027),
                               salt=90))
    ids = [c["id"] for c in cases]
    assert len(set(ids)) == len(ids), sorted(
        i for i in set(ids) if ids.count(i) > 1)
    return cases


# ---------------------------------------------------------------------------
# One rank's walk through the table (runs inside an executor thread)
# ---------------------------------------------------------------------------


def _pattern(total):
    return (np.arange(total, dtype=np.uint32) * 7 + 3).astype(np.uint8)


class _Buf:
    """nbytes of payload between two guard bands, on the device or (for the
    mixed sendRecv cases) on the host. `ptr` is the payload's address, off
    bytes past 16 B alignment. Without a payload the buffer holds the guard
    pattern throughout, which is what an untouched buffer must still hold."""

    def __init__(self, nbytes, payload=None, off=0, host=False):
        self.lead = GUARD + off
        self.nbytes = nbytes
        self.initial = _pattern(self.lead + nbytes + GUARD)
        if payload is not None:
            raw = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
            assert raw.size == nbytes
            self.initial[self.lead:self.lead + nbytes] = raw
        self.host = host
        if host:
            self.mem = self.initial.copy()
            base = self.mem.ctypes.data
        else:
            self.mem = torch.from_numpy(self.initial.copy()).to("cuda")
            base = self.mem.data_ptr()
            assert base % 16 == 0
        self.ptr = base + self.lead

    def read(self):
        return self.mem.copy() if self.host else self.mem.cpu().numpy()

    def payload(self, raw, dtype):
        return raw[self.lead:self.lead + self.nbytes].copy().view(
            km.NP_DTYPE[dtype])


class _Rank:
    def __init__(self, core, rank, size):
        self.c = core
        self.rank = rank
        self.size = size
        self.bad = []

    def note(self, case, what, miss):
        self.bad.append([case["id"], "rank%d %s" % (self.rank, what),
                         *[str(m) for m in miss]])

    def check(self, case, what, buf, want, op=None):
        """Guards untouched and payload equal to `want` (None: untouched)."""
        raw = buf.read()
        dtype = case["dtype"]
        if want is None:
            want = buf.payload(buf.initial, dtype)
            op = None
        miss = mm.first_mismatch(dtype, op, buf.payload(raw, dtype),
                                 np.asarray(want))
        if miss is not None:
            self.note(case, what, miss)
        end = buf.lead + buf.nbytes
        for name, sl in (("front guard", slice(0, buf.lead)),
                         ("back guard", slice(end, None))):
            g = mm.first_mismatch(km.DT_BYTE, None, raw[sl], buf.initial[sl])
            if g is not None:
                self.note(case, what + " " + name, g)

    def run(self, case):
        getattr(self, "_" + case["kind"])(case)

    # -- reducing collectives ------------------------------------------------

    def _reducing(self, case, recv_count, total):
        c, r, size = self.c, self.rank, self.size
        dtype, op, n = case["dtype"], case["op"], case["n"]
        isz = km.NP_DTYPE[dtype].itemsize
        xs = mm.reduce_inputs(dtype, op, size, total, case["salt"])
        send = _Buf(total * isz, xs[r], case["send_off"])
        recv = send if case["inplace"] else _Buf(recv_count * isz, None,
                                                 case["recv_off"])
        torch.cuda.synchronize()
        mdt, mop = c.MpiDataType(dtype), c.MpiOp(op)
        kind = case["kind"]
        if kind == "reduce":
            c.mpi_reduce_ptr(r, case["root"], send.ptr, recv.ptr, n, mdt, mop)
            want = mm.reduce_model(dtype, op, xs, case["root"])[r]
        elif kind == "allreduce":
            c.mpi_allreduce_ptr(r, send.ptr, recv.ptr, n, mdt, mop)
            want = mm.allreduce_model(dtype, op, xs)[r]
        elif kind == "scan":
            c.mpi_scan_ptr(r, send.ptr, recv.ptr, n, mdt, mop)
            want = mm.scan_model(dtype, op, xs)[r]
        else:
            c.mpi_reducescatter_ptr(r, send.ptr, recv.ptr, n, mdt, mop)
            want = mm.reducescatter_model(dtype, op, xs, n)[r]
        # a rank that receives nothing keeps what its buffer held
        self.check(case, "recv", recv, want, op)
        if recv is not send:
            self.check(case, "send", send, None)

    def _reduce(self, case):
        self._reducing(case, case["n"], case["n"])

    _allreduce = _reduce
    _scan = _reduce

    def _reducescatter(self, case):
        self._reducing(case, case["n"], case["n"] * self.size)

    # -- data movers -----------------------------------------------------------

    def _ring(self):
        return (self.rank + 1) % self.size, (self.rank - 1) % self.size

    def _p2p_bufs(self, case, send_host=False, recv_host=False):
        dtype, n = case["dtype"], case["n"]
        nbytes = n * km.NP_DTYPE[dtype].itemsize
        xs = mm.mover_inputs(dtype, self.size, n, case["salt"])
        send = _Buf(nbytes, xs[self.rank], case["send_off"], host=send_host)
        recv = _Buf(nbytes, None, case["recv_off"], host=recv_host)
        torch.cuda.synchronize()
        return xs, send, recv

    def _sendrecv_ring(self, case, send_host=False, recv_host=False):
        xs, send, recv = self._p2p_bufs(case, send_host, recv_host)
        nxt, prv = self._ring()
        self.c.mpi_sendrecv_ptr(self.rank, nxt, prv, send.ptr, recv.ptr,
                                case["n"], self.c.MpiDataType(case["dtype"]))
        self.check(case, "recv", recv, xs[prv])
        self.check(case, "send", send, None)

    def _sendrecv_host_to_dev(self, case):
        self._sendrecv_ring(case, send_host=True)

    def _sendrecv_dev_to_host(self, case):
        self._sendrecv_ring(case, recv_host=True)

    def _send_recv(self, case):
        xs, send, recv = self._p2p_bufs(case)
        nxt, prv = self._ring()
        mdt = self.c.MpiDataType(case["dtype"])
        # device-plane sends are buffered, so the ring cannot deadlock
        self.c.mpi_send_ptr(self.rank, nxt, send.ptr, case["n"], mdt)
        self.c.mpi_recv_ptr(prv, self.rank, recv.ptr, case["n"], mdt)
        self.check(case, "recv", recv, xs[prv])
        self.check(case, "send", send, None)

    def _isend_irecv(self, case):
        xs, send, recv = self._p2p_bufs(case)
        nxt, prv = self._ring()
        mdt = self.c.MpiDataType(case["dtype"])
        rreq = self.c.mpi_irecv_ptr(prv, self.rank, recv.ptr, case["n"], mdt)
        sreq = self.c.mpi_isend_ptr(self.rank, nxt, send.ptr, case["n"], mdt)
        self.c.mpi_await(sreq)
        self.c.mpi_await(rreq)
        self.check(case, "recv", recv, xs[prv])
        self.check(case, "send", send, None)

    def _order(self, case, second_is_irecv):
        """Rank 0 posts two different messages to the last rank on one
        channel; the receiver's first posted receive must get the first."""
        c, r = self.c, self.rank
        dtype, n = case["dtype"], case["n"]
        nbytes = n * km.NP_DTYPE[dtype].itemsize
        mdt = c.MpiDataType(dtype)
        first = mm.mover_input(dtype, 0, n, case["salt"])
        second = mm.mover_input(dtype, 1, n, case["salt"])
        assert not np.array_equal(km.bits(first), km.bits(second))
        sender, receiver = 0, self.size - 1
        if r == sender:
            for data in (first, second):
                buf = _Buf(nbytes, data)
                torch.cuda.synchronize()
                c.mpi_send_ptr(sender, receiver, buf.ptr, n, mdt)
        if r == receiver:
            a = _Buf(nbytes, None)
            b = _Buf(nbytes, None)
            torch.cuda.synchronize()
            req_a = c.mpi_irecv_ptr(sender, receiver, a.ptr, n, mdt)
            if second_is_irecv:
                req_b = c.mpi_irecv_ptr(sender, receiver, b.ptr, n, mdt)
                c.mpi_await(req_b)
            else:
                c.mpi_recv_ptr(sender, receiver, b.ptr, n, mdt)
            c.mpi_await(req_a)
            self.check(case, "A (posted first)", a, first)
            self.check(case, "B (posted second)", b, second)

    def _order_irecv_recv(self, case):
        self._order(case, False)

    def _order_irecv_irecv(self, case):
        self._order(case, True)

    def _bcast(self, case):
        dtype, n, root = case["dtype"], case["n"], case["root"]
        xs = mm.mover_inputs(dtype, self.size, n, case["salt"])
        buf = _Buf(n * km.NP_DTYPE[dtype].itemsize, xs[self.rank],
                   case["recv_off"])
        torch.cuda.synchronize()
        self.c.mpi_bcast_ptr(root, self.rank, buf.ptr, n,
                             self.c.MpiDataType(dtype))
        self.check(case, "buffer", buf, mm.broadcast_model(xs, root)[self.rank])

    def _allgather(self, case):
        dtype, n, r, size = case["dtype"], case["n"], self.rank, self.size
        isz = km.NP_DTYPE[dtype].itemsize
        xs = mm.mover_inputs(dtype, size, n, case["salt"])
        if case["inplace"]:
            # own contribution already at recv + rank * bytes
            filler = mm.mover_inputs(dtype, size, n, case["salt"] + 1000)
            filler[r] = xs[r]
            recv = _Buf(n * size * isz, np.concatenate(filler))
            send_ptr = recv.ptr + r * n * isz
            send = None
        else:
            recv = _Buf(n * size * isz, None, case["recv_off"])
            send = _Buf(n * isz, xs[r], case["send_off"])
            send_ptr = send.ptr
        torch.cuda.synchronize()
        self.c.mpi_allgather_ptr(r, send_ptr, recv.ptr, n,
                                 self.c.MpiDataType(dtype))
        self.check(case, "recv", recv, mm.allgather_model(xs)[r])
        if send is not None:
            self.check(case, "send", send, None)

    def _alltoall(self, case):
        dtype, n, r, size = case["dtype"], case["n"], self.rank, self.size
        isz = km.NP_DTYPE[dtype].itemsize
        xs = mm.mover_inputs(dtype, size, n * size, case["salt"])
        send = _Buf(n * size * isz, xs[r], case["send_off"])
        recv = _Buf(n * size * isz, None, case["recv_off"])
        torch.cuda.synchronize()
        self.c.mpi_alltoall_ptr(r, send.ptr, recv.ptr, n,
                                self.c.MpiDataType(dtype))
        self.check(case, "recv", recv, mm.alltoall_model(xs, n)[r])
        self.check(case, "send", send, None)

    def _scatter(self, case):
        dtype, n, r, size = case["dtype"], case["n"], self.rank, self.size
        root = case["root"]
        isz = km.NP_DTYPE[dtype].itemsize
        xs = mm.mover_inputs(dtype, size, n * size, case["salt"])
        # only the root's send buffer is significant
        send = _Buf(n * size * isz, xs[r], case["send_off"]) \
            if r == root else None
        recv = _Buf(n * isz, None, case["recv_off"])
        torch.cuda.synchronize()
        self.c.mpi_scatter_ptr(root, r, send.ptr if send else 0, recv.ptr, n,
                               self.c.MpiDataType(dtype))
        self.check(case, "recv", recv, mm.scatter_model(xs, root, n)[r])
        if send is not None:
            self.check(case, "send", send, None)

    def _gather(self, case):
        dtype, n, r, size = case["dtype"], case["n"], self.rank, self.size
        root = case["root"]
        isz = km.NP_DTYPE[dtype].itemsize
        xs = mm.mover_inputs(dtype, size, n, case["salt"])
        send = _Buf(n * isz, xs[r], case["send_off"])
        # only the root's receive buffer is significant
        recv = _Buf(n * size * isz, None, case["recv_off"]) \
            if r == root else None
        torch.cuda.synchronize()
        self.c.mpi_gather_ptr(r, root, send.ptr, recv.ptr if recv else 0, n,
                              self.c.MpiDataType(dtype))
        if recv is not None:
            self.check(case, "recv", recv, mm.gather_model(xs, root)[r])
        self.check(case, "send", send, None)


def _table_fn(msg):
    """The function every rank executes: the whole table, then the list of
    mismatches as JSON. An exception leaves the ranks out of step, so the
    rank stops there and says where."""
    from faabric_amd import _core

    _, rank, size = _core.mpi_init()
    run = _Rank(_core, rank, size)
    done = 0
    try:
        for case in device_cases(size):
            run.run(case)
            done += 1
        _core.mpi_barrier(rank)
    except Exception as e:  # noqa: BLE001 - reported, never swallowed
        run.bad.append([device_cases(size)[done]["id"],
                        "rank%d exception" % rank, repr(e)])
    finally:
        _core.mpi_finalize()
    msg.output_data = json.dumps({"cases": done, "bad": run.bad[:200]})
    return 1 if run.bad else 0


# ---------------------------------------------------------------------------
# Launches
# ---------------------------------------------------------------------------


def _child_setup():
    """Before the package is imported: the plane is chosen once per process."""
    assert "faabric_amd" not in sys.modules
    os.environ["FAABRIC_DEVICE_PLANE"] = "ptp"
    os.environ["FAABRIC_IPC_ARENA_MB"] = "64"
    # a rank that stopped early must not keep its peers waiting for long
    os.environ["GLOBAL_MESSAGE_TIMEOUT"] = "20000"
    sys.path.insert(0, REPO_ROOT)


def _submit(core, wait_for_batch, size, hosts=None):
    ber = core.batch_exec_factory("devplane", "table", 1)
    msgs = ber.messages
    msgs[0].is_mpi = True
    msgs[0].mpi_world_size = size
    ber.messages = msgs
    if hosts is not None:
        # gang-place rank r on worker r
        d = core.SchedulingDecision()
        d.app_id = ber.app_id
        d.group_id = 0
        d.hosts = hosts
        d.message_ids = [0] * size
        d.app_idxs = list(range(size))
        d.group_idxs = list(range(size))
        d.mpi_ports = [0] * size
        d.n_functions = size
        core.preload_scheduling_decision(ber.app_id, d)
    core.call_functions(ber)
    t0 = time.monotonic()
    results = wait_for_batch(ber.app_id, size, 120_000)
    return {
        "seconds": time.monotonic() - t0,
        "ranks": [(r.mpi_rank, r.return_value, r.output_data,
                   r.executed_host) for r in results],
    }


def _inproc_child(result_q):
    _child_setup()
    try:
        import torch as t  # noqa: F401
        from faabric_amd import _core
        from faabric_amd.runtime import LocalRuntime, wait_for_batch

        _core.set_log_level("error")
        rt = LocalRuntime(port_offset=INPROC_OFFSET,
                          planner_port_offset=INPROC_OFFSET,
                          slots=max(INPROC_SIZES))
        rt.start_planner(with_snapshot_server=False)
        rt.start_worker()
        _core.register_function("devplane", "table", _table_fn)
        out = {}
        try:
            for size in INPROC_SIZES:
                out[size] = _submit(_core, wait_for_batch, size)
        finally:
            rt.stop()
        result_q.put(("ok", out))
    except Exception as e:  # noqa: BLE001
        result_q.put(("error", repr(e)))


def _cross_child(rank, stop, ready, result_q):
    _child_setup()
    try:
        import torch as t  # noqa: F401
        from faabric_amd import _core
        from faabric_amd.runtime import LocalRuntime, wait_for_batch

        _core.set_log_level("error")
        rt = LocalRuntime(port_offset=CROSS_BASE + rank * CROSS_STEP,
                          planner_port_offset=CROSS_BASE, slots=1)
        if rank == 0:
            rt.start_planner(with_snapshot_server=False)
        rt.start_worker()
        _core.register_function("devplane", "table", _table_fn)
        ready.set()
        try:
            if rank == 0:
                deadline = time.monotonic() + 60
                while (time.monotonic() < deadline
                       and len(_core.get_available_hosts()) < CROSS_SIZE):
                    time.sleep(0.05)
                assert len(_core.get_available_hosts()) == CROSS_SIZE
                hosts = ["127.0.0.1@%d" % (CROSS_BASE + r * CROSS_STEP)
                         for r in range(CROSS_SIZE)]
                out = _submit(_core, wait_for_batch, CROSS_SIZE, hosts)
                out["ipc_available"] = bool(_core.ipc_available(hosts[1]))
                out["ipc_shipped"] = tuple(_core.ipc_shipped())
                result_q.put(("ok", out))
            stop.wait(200)
        finally:
            rt.stop()
    except Exception as e:  # noqa: BLE001
        result_q.put(("error", repr(e)))
        ready.set()


def _join(procs, seconds):
    """Wait for the children within one shared time limit and return their
    exit codes (None for one that had to be killed)."""
    deadline = time.monotonic() + seconds
    codes = []
    for p in procs:
        p.join(timeout=max(0.0, deadline - time.monotonic()))
        if p.is_alive():
            p.kill()
            p.join(timeout=10)
            codes.append(None)
        else:
            codes.append(p.exitcode)
    return codes


# A child that faulted, aborted or hung: nothing more is started on the GPU.
_gpu_unsafe = []


def _launch_guard():
    if _gpu_unsafe:
        pytest.fail("not started: an earlier launch ended badly: %s"
                    % _gpu_unsafe)


@pytest.fixture(scope="module")
def inproc():
    _launch_guard()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_inproc_child, args=(q,))
    t0 = time.monotonic()
    p.start()
    try:
        status, out = q.get(timeout=240)
    except Exception:  # queue.Empty: the child hung or died silently
        status, out = "error", "no result from the child"
    codes = _join([p], 60)
    if codes != [0]:
        _gpu_unsafe.append(("in-process child exit", codes))
    assert codes == [0], (codes, status, out)
    assert status == "ok", out
    out["wall"] = time.monotonic() - t0
    return out


@pytest.fixture(scope="module")
def cross():
    _launch_guard()
    ctx = mp.get_context("spawn")
    stop = ctx.Event()
    q = ctx.Queue()
    procs, readies = [], []
    t0 = time.monotonic()
    for r in range(CROSS_SIZE):
        ready = ctx.Event()
        p = ctx.Process(target=_cross_child, args=(r, stop, ready, q))
        p.start()
        procs.append(p)
        readies.append(ready)
    try:
        started = all(ready.wait(120) for ready in readies)
        try:
            status, out = q.get(timeout=240) if started else (
                "error", "a worker failed to start")
        except Exception:  # queue.Empty
            status, out = "error", "no result from the workers"
    finally:
        stop.set()
        codes = _join(procs, 60)
    if codes != [0] * CROSS_SIZE:
        _gpu_unsafe.append(("cross-process worker exit", codes))
    assert codes == [0] * CROSS_SIZE, (codes, status, out)
    assert status == "ok", out
    out["wall"] = time.monotonic() - t0
    return out


# ---------------------------------------------------------------------------
# Assertions on what the launches recorded
# ---------------------------------------------------------------------------


def _bad_by_case(run, size):
    """case id -> mismatches; asserts that every rank walked the table."""
    n_cases = len(device_cases(size))
    ranks = run["ranks"]
    assert sorted(r[0] for r in ranks) == list(range(size)), ranks
    bad = {}
    for rank, rc, output, _host in ranks:
        rec = json.loads(output)
        for entry in rec["bad"]:
            bad.setdefault(entry[0], []).append(entry[1:])
        assert rec["cases"] == n_cases or rec["bad"], (rank, rec)
        assert (rc == 0) == (not rec["bad"]), (rank, rc, rec)
    return bad


def _assert_group_clean(bad, pred, size):
    ids = [c["id"] for c in device_cases(size) if pred(c)]
    assert ids
    failed = {i: bad[i] for i in ids if i in bad}
    assert not failed, "%d of %d cases differ from the model: %s; first: %s" % (
        len(failed), len(ids), sorted(failed), next(iter(failed.items())))


_GROUPS = {
    "reduce": lambda c: c["kind"] == "reduce",
    "allreduce": lambda c: c["kind"] == "allreduce",
    "scan": lambda c: c["kind"] == "scan",
    "reducescatter": lambda c: c["kind"] == "reducescatter",
    "p2p": lambda c: c["kind"] in ("send_recv", "isend_irecv",
                                   "sendrecv_ring"),
    "bcast": lambda c: c["kind"] == "bcast",
    "allgather": lambda c: c["kind"] == "allgather",
    "alltoall": lambda c: c["kind"] == "alltoall",
    "scatter": lambda c: c["kind"] == "scatter",
    "gather": lambda c: c["kind"] == "gather",
    "matching_order": lambda c: c["kind"].startswith("order_"),
    "sendrecv_mixed": lambda c: c["kind"] in ("sendrecv_host_to_dev",
                                              "sendrecv_dev_to_host"),
}


@pytest.mark.parametrize("group", sorted(_GROUPS))
@pytest.mark.parametrize("size", INPROC_SIZES)
def test_in_process_plane(inproc, size, group):
    bad = _bad_by_case(inproc[size], size)
    _assert_group_clean(bad, _GROUPS[group], size)


def test_in_process_plane_no_stray_mismatch(inproc):
    """Nothing recorded under an id outside the table, and the whole module's
    launch stays quick."""
    for size in INPROC_SIZES:
        bad = _bad_by_case(inproc[size], size)
        assert set(bad) <= {c["id"] for c in device_cases(size)}
        print("in-process world %d: %.2f s" % (size, inproc[size]["seconds"]))
    print("in-process launch: %.2f s" % inproc["wall"])


@pytest.mark.parametrize("group", sorted(_GROUPS))
def test_cross_process_plane(cross, group):
    bad = _bad_by_case(cross, CROSS_SIZE)
    _assert_group_clean(bad, _GROUPS[group], CROSS_SIZE)


def test_cross_process_plane_spans_workers(cross):
    hosts = {r[3] for r in cross["ranks"]}
    assert len(hosts) == CROSS_SIZE, hosts
    if not cross["ipc_available"]:
        pytest.skip("no HIP-IPC arena between the workers: the table ran "
                    "over the staged RPC path only")
    segments, nbytes = cross["ipc_shipped"]
    assert segments > 0 and nbytes > 0
    print("cross-process world: %.2f s, launch %.2f s"
          % (cross["seconds"], cross["wall"]))


def test_case_table_covers_the_issue():
    for size in (1, 2, 3):
        cases = device_cases(size)
        for kind in REDUCERS:
            assert {(c["dtype"], c["op"]) for c in cases
                    if c["kind"] == kind} == set(mm.DTYPE_OP_PAIRS)
            assert {c["n"] for c in cases if c["kind"] == kind} >= {
                0, 1, 257, 1027, 4099, 65537}
        for kind in MOVERS:
            assert {c["dtype"] for c in cases
                    if c["kind"] == kind} == set(mm.DTYPES)
            assert {c["n"] for c in cases if c["kind"] == kind} >= {
                0, 1, 257, 1027, 4099, 65537}
        for kind in ("reduce", "bcast", "scatter", "gather"):
            assert {c["root"] for c in cases
                    if c["kind"] == kind} == set(roots(size))
        assert {c["kind"] for c in cases if c["inplace"]} == {
            "reduce", "allreduce", "scan", "allgather"}
        assert {(c["send_off"], c["recv_off"]) for c in cases} == {
            (0, 0), (4, 0), (0, 4), (4, 4)}
        assert max(c["n"] for c in cases) <= 66000
        assert (1027 * 4) % 16 and (1027 * 8) % 16 and 4099 % 16
