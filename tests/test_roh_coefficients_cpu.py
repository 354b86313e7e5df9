"""kgx_roh_coefficients (host only): F_ROH = total_length / denominator, one IEEE division -- the bits of numpy's."""
import numpy as np
import pytest

from kgl_gene_amd import capi


@pytest.mark.parametrize("denominator", [1, 3, 2_900_000_000, (1 << 53) + 1, (1 << 64) - 1])
def test_one_division(denominator):
    summary = np.zeros(6, dtype=capi.ROH_SUMMARY)
    summary["total_length"] = [0, 1, 7, 123_456_789, (1 << 53) + 3, (1 << 64) - 1]
    got = capi.roh_coefficients(summary, denominator)
    want = summary["total_length"].astype(np.float64) / np.float64(np.uint64(denominator))
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_no_denominator_is_nan():
    summary = np.zeros(3, dtype=capi.ROH_SUMMARY)
    summary["total_length"] = [0, 5, 9]
    assert np.isnan(capi.roh_coefficients(summary, 0)).all()
