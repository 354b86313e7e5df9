"""kgx_pair_run_fractions (host only): total_length / denominator per pair, one IEEE division -- the bits of numpy's -- in the order
of the pair index."""
import numpy as np
import pytest

from kgl_gene_amd import capi

G = 3
TOTALS = [0, 1, 7, 123_456_789, (1 << 53) + 3, (1 << 64) - 1]      # G (G + 1) / 2 pairs


def table():
    summary = np.zeros((len(TOTALS), 4), dtype=np.uint64)
    summary[:, 1] = TOTALS
    summary[:, [0, 2, 3]] = 99                                     # the other words do not enter
    return summary


@pytest.mark.parametrize("denominator", [1, 3, 2_900_000_000, (1 << 53) + 1, (1 << 64) - 1])
def test_one_division(denominator):
    got = capi.pair_run_fractions(table(), G, denominator)
    want = np.array(TOTALS, dtype=np.uint64).astype(np.float64) / np.float64(np.uint64(denominator))
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_no_denominator_is_nan():
    assert np.isnan(capi.pair_run_fractions(table(), G, 0)).all()


def test_pair_index_order():
    got = capi.pair_run_fractions(table(), G, 1)
    for p, (a, b) in enumerate(zip(*np.triu_indices(G))):          # row-major over a <= b
        assert capi.pair_index(int(a), int(b), G) == p and got[p] == float(TOTALS[p])
    assert capi.KGX_SHARE_IBS0 == 0 and capi.KGX_SHARE_IDENTICAL == 1
    with pytest.raises(ValueError):
        capi.pair_run_fractions(table()[:5], G, 1)
