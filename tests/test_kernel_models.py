"""The numpy reference models in kernel_models.py, pinned on the CPU: the
elementwise model against the host plane's op_reduce (opReduceLoop in
cpp/src/mpi.cpp), bit for bit, and the xorshift/diff models against values
worked out by hand. Needs no GPU."""

import numpy as np
import pytest

import kernel_models as km
from faabric_amd import _core

HOST_OPS = [km.OP_SUM, km.OP_MAX, km.OP_MIN, km.OP_PROD]


@pytest.mark.parametrize("dtype", sorted(km.NP_DTYPE), ids=km.DTYPE_NAME.get)
@pytest.mark.parametrize("op", HOST_OPS, ids=km.OP_NAME.get)
def test_elementwise_model_equals_host_plane(dtype, op):
    inout, inp = km.operand_pairs(dtype, op)
    assert inout.size == inp.size and inout.size > 0
    want = km.elementwise_model(op, dtype, inout, inp)
    got = np.frombuffer(
        _core._debug_op_reduce_host(op, dtype, inp.tobytes(), inout.tobytes()),
        dtype=km.NP_DTYPE[dtype],
    )
    assert np.array_equal(km.bits(got), km.bits(want)), [
        (hex(int(a)), hex(int(b)), hex(int(g)), hex(int(w)))
        for a, b, g, w in zip(km.bits(inout), km.bits(inp), km.bits(got),
                              km.bits(want))
        if g != w
    ][:8]


def test_host_plane_binding_rejects_bad_arguments():
    four = b"\x00" * 4
    with pytest.raises(RuntimeError):
        _core._debug_op_reduce_host(km.OP_SUB, km.DT_INT32, four, four)
    with pytest.raises(RuntimeError):
        _core._debug_op_reduce_host(km.OP_SUM, 6, four, four)
    with pytest.raises(RuntimeError):
        _core._debug_op_reduce_host(km.OP_SUM, km.DT_INT32, four, four * 2)
    with pytest.raises(RuntimeError):
        _core._debug_op_reduce_host(km.OP_SUM, km.DT_INT64, four, four)


@pytest.mark.parametrize("dtype", sorted(km.NP_DTYPE), ids=km.DTYPE_NAME.get)
def test_operand_pairs_cover_every_pairing(dtype):
    vals = km.adversarial_values(dtype)
    inout, inp = km.operand_pairs(dtype, km.OP_MAX)
    seen = set(zip(km.bits(inout).tolist(), km.bits(inp).tolist()))
    vb = km.bits(vals).tolist()
    assert len(set(vb)) == len(vb)
    assert seen == {(a, b) for a in vb for b in vb}
    # all pairings fit the longest elementwise test length
    assert inout.size <= 513


def test_signed_pairings_leave_out_only_overflow():
    for dtype in (km.DT_INT32, km.DT_INT64):
        ii = np.iinfo(km.NP_DTYPE[dtype])
        full = km.operand_pairs(dtype, km.OP_MAX)[0].size
        for op, fn in ((km.OP_SUM, lambda a, b: a + b),
                       (km.OP_SUB, lambda a, b: a - b),
                       (km.OP_PROD, lambda a, b: a * b)):
            inout, inp = km.operand_pairs(dtype, op)
            exact = [fn(int(a), int(b)) for a, b in zip(inout, inp)]
            assert all(ii.min <= r <= ii.max for r in exact)
            assert 0 < inout.size < full
            # the extremes stay in: min + max, max - max, min * 1
            pairs = set(zip(inout.tolist(), inp.tolist()))
            assert {km.OP_SUM: (ii.min, ii.max),
                    km.OP_SUB: (ii.max, ii.max),
                    km.OP_PROD: (ii.min, 1)}[op] in pairs


def test_model_max_min_operand_order():
    """Ties and NaN keep inout, as std::max/std::min(inout, in) do."""
    for dtype in (km.DT_FLOAT, km.DT_DOUBLE):
        ft = km.NP_DTYPE[dtype]
        nan = ft.type("nan")
        inout = np.array([0.0, -0.0, nan, 1.0], dtype=ft)
        inp = np.array([-0.0, 0.0, 1.0, nan], dtype=ft)
        for op in (km.OP_MAX, km.OP_MIN):
            got = km.elementwise_model(op, dtype, inout, inp)
            assert np.array_equal(km.bits(got), km.bits(inout))


def test_model_unsigned_wrap_and_order():
    a = np.array([2**64 - 1, 0, 2**63, 2**63 - 1], dtype=np.uint64)
    b = np.array([1, 1, 2, 2**63], dtype=np.uint64)
    assert km.elementwise_model(km.OP_SUM, km.DT_UINT64, a, b).tolist() == [
        0, 1, 2**63 + 2, 2**64 - 1]
    assert km.elementwise_model(km.OP_SUB, km.DT_UINT64, a, b).tolist() == [
        2**64 - 2, 2**64 - 1, 2**63 - 2, 2**64 - 1]
    assert km.elementwise_model(km.OP_PROD, km.DT_UINT64, a, b).tolist() == [
        2**64 - 1, 0, 0, 2**63]
    assert km.elementwise_model(km.OP_MAX, km.DT_UINT64, a, b).tolist() == [
        2**64 - 1, 1, 2**63, 2**63]
    assert km.elementwise_model(km.OP_MIN, km.DT_UINT64, a, b).tolist() == [
        1, 0, 2, 2**63 - 1]
    x = np.array([200, 255, 0], dtype=np.uint8)
    y = np.array([100, 255, 1], dtype=np.uint8)
    assert km.elementwise_model(km.OP_SUM, km.DT_BYTE, x, y).tolist() == [
        44, 254, 1]
    assert km.elementwise_model(km.OP_SUB, km.DT_BYTE, y, x).tolist() == [
        156, 0, 1]
    assert km.elementwise_model(km.OP_XOR, km.DT_BYTE, x, y).tolist() == [
        172, 0, 1]
    with pytest.raises(ValueError):
        km.elementwise_model(km.OP_XOR, km.DT_INT32, [1], [1])


def _xorshift64_int(x):
    m = (1 << 64) - 1
    x ^= (x << 13) & m
    x ^= x >> 7
    x ^= (x << 17) & m
    return x


def test_xorshift_models_match_integer_arithmetic():
    # Marsaglia's xorshift64 (13, 7, 17) from state 1
    assert _xorshift64_int(1) == 0x40822041
    xs = [0, 1, 2**63, 2**64 - 1, 0x9E3779B97F4A7C15, 12345678901234567]
    assert km.xorshift64(np.array(xs, dtype=np.uint64)).tolist() == [
        _xorshift64_int(x) for x in xs]

    m = (1 << 64) - 1
    seed = 0xDEADBEEFCAFEF00D
    n = 1030
    want = [
        _xorshift64_int(seed ^ ((i * 0x9E3779B97F4A7C15) & m) ^ (i >> 3))
        for i in range(n)
    ]
    assert km.fill_random_model(n, seed).tolist() == want

    words = km.fill_random_model(4 * 512, 3)
    got = km.touch_pages_model(words, [2, 0], seed)
    exp = words.tolist()
    for p in (0, 2):
        for w in range(p * 512, (p + 1) * 512):
            exp[w] ^= _xorshift64_int(seed ^ w)
    assert got.tolist() == exp
    assert np.array_equal(got[512:1024], words[512:1024])


def test_diff_models():
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, 70 * km.PAGE, dtype=np.uint8)
    assert km.dirty_set_model(base, base) == []
    for name, pages in km.dirty_patterns(70).items():
        upd = km.flip_pages(base, pages)
        assert km.dirty_set_model(base, upd) == pages, name
        pl = km.payload_model(base, upd)
        assert int(np.count_nonzero(pl)) == len(pages)
        # one bit per dirty page
        assert sorted(set(np.nonzero(pl)[0].tolist())) == pages
        assert all(bin(int(v)).count("1") == 1 for v in pl[pl != 0])
    assert "31_32" in km.dirty_patterns(33)
    assert "31_32" not in km.dirty_patterns(32)
    assert "2047_2048" in km.dirty_patterns(2049)
    assert "2047_2048" not in km.dirty_patterns(2048)
