"""Device-KV dirty-bitmap sweep (CPU): the sweep that turns the per-page
dirty bitmap into the commit kernel's page list must return exactly the
set bits, ascending, and leave the bitmap all zero — across 64-bit word
boundaries and in a partial last word."""

import pytest

from faabric_amd import _core

SIZES = [1, 63, 64, 65, 130]


def sweep(n_pages, bits):
    pages, after = _core._debug_kv_sweep_bitmap(n_pages, list(bits))
    assert len(after) == (n_pages + 63) // 64
    assert all(w == 0 for w in after), after
    return pages


@pytest.mark.parametrize("n_pages", SIZES)
def test_sweep_no_bits(n_pages):
    assert sweep(n_pages, []) == []


@pytest.mark.parametrize("n_pages", SIZES)
def test_sweep_all_bits(n_pages):
    assert sweep(n_pages, range(n_pages)) == list(range(n_pages))


@pytest.mark.parametrize("n_pages", SIZES)
def test_sweep_last_valid_bit(n_pages):
    assert sweep(n_pages, [n_pages - 1]) == [n_pages - 1]


@pytest.mark.parametrize("n_pages", SIZES)
def test_sweep_first_and_last(n_pages):
    want = sorted({0, n_pages - 1})
    assert sweep(n_pages, want) == want


@pytest.mark.parametrize("n_pages", SIZES)
def test_sweep_scattered_unordered_input(n_pages):
    # Every third page plus the bits either side of each word boundary,
    # handed over in descending order: the list still comes back ascending
    want = set(range(0, n_pages, 3))
    for edge in (62, 63, 64, 65, 126, 127, 128, 129):
        if edge < n_pages:
            want.add(edge)
    assert sweep(n_pages, sorted(want, reverse=True)) == sorted(want)


def test_sweep_duplicates_collapse():
    assert sweep(130, [64, 64, 5, 129, 5]) == [5, 64, 129]
