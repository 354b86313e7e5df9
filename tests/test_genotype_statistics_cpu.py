"""kgx_genotype_statistics (host only, no device) against a Python restatement of GenotypeAnalysis::Gini / HRel / IQV
(kga_analytic/kga_PfEMP/kga_analysis_PfEMP_variant.cpp:499-628) in the reference's own operation order, quirks included: the
zero-variant genomes are one more category even when there are none, IQV's proportions are divided by total x 100, and without a
genotype Gini and IQV are 1.0 and HRel 0.0.

Tolerances (derived, not measured):
  Gini, IQV  1e-15 relative: Gini's sum of |f_i - f_j| is an exactly representable integer however it is added up, so the
             library's integer form and the reference's double loop differ by nothing before the three roundings that follow
             (the scaling, the product, the subtraction); IQV is restated operation for operation.
  HRel       1e-12 absolute: at most one ulp of log2 per term, over at most ~10^3 terms each below 0.54 in magnitude, for a
             result in [0, 1].
"""
import math

import numpy as np
import pytest

from kgl_gene_amd import capi


@pytest.fixture(scope="module")
def stats():
    capi.ensure_built()
    return capi.genotype_statistics


def reference_statistics(counts, zero):
    """The three functions as the reference writes them; counts in std::map order."""
    counts = [int(c) for c in counts]
    categories = len(counts) + 1
    if categories <= 1:
        return 1.0, 0.0, 1.0
    total = zero + sum(counts)
    freq = [float(zero)] + [float(c) for c in counts]
    s = 0.0
    for i in range(categories - 1):
        fi = freq[i]
        for j in range(i + 1, categories):
            s += math.fabs(fi - freq[j])
    scaling = 1.0 / (float(total) * float(categories - 1))
    gini = 1.0 - (scaling * s)
    h = 0.0
    if zero:
        p = float(zero) / float(total)
        h = math.log2(p) * p
    for c in counts:
        p = float(c) / float(total)
        h += math.log2(p) * p
    hrel = (-1.0 * h) / math.log2(categories)
    p = float(zero) / (float(total) * 100.0)
    q = p * p
    for c in counts:
        p = float(c) / (float(total) * 100.0)
        q += p * p
    iqv = (float(categories) / float(categories - 1)) * (1.0 - q)
    return gini, hrel, iqv


def check(stats, counts, zero):
    got = stats(np.asarray(counts, dtype=np.uint32), zero)
    want = reference_statistics(counts, zero)
    print(f"k={len(counts)} zero={zero}: got {got} want {want}")
    assert got[0] == pytest.approx(want[0], rel=1e-15, abs=0.0)
    assert got[1] == pytest.approx(want[1], rel=0.0, abs=1e-12)
    assert got[2] == pytest.approx(want[2], rel=1e-15, abs=0.0)
    return got


def test_no_genotype_at_all(stats):
    assert stats(np.zeros(0, dtype=np.uint32), 0) == (1.0, 0.0, 1.0)
    assert stats(np.zeros(0, dtype=np.uint32), 1234) == (1.0, 0.0, 1.0)


def test_a_single_genotype_with_and_without_zero_variant_genomes(stats):
    gini, hrel, iqv = check(stats, [40], 0)
    # two categories, one of them empty: |40 - 0| / (40 * 1) = 1 -> Gini 0; no entropy; IQV = 2 (1 - (1/100)^2)
    assert gini == 0.0 and hrel == 0.0 and iqv == 2.0 * (1.0 - 0.01 * 0.01)
    gini, hrel, iqv = check(stats, [40], 40)
    assert gini == 1.0 and hrel == 1.0
    check(stats, [7], 93)


def test_all_counts_equal(stats):
    gini, hrel, _ = check(stats, [5] * 99, 5)
    assert gini == 1.0 and hrel == pytest.approx(1.0, abs=1e-12)
    check(stats, [5] * 99, 0)       # the empty extra category alone makes it unequal


def test_a_thousand_random_counts(stats):
    rng = np.random.default_rng(20261)
    counts = rng.integers(1, 5000, 1000)
    check(stats, counts, 0)
    check(stats, counts, 321)
    # the order given is the order HRel is summed in: the same multiset in another order may differ in the last bits only
    a = check(stats, counts[::-1], 321)
    b = check(stats, np.sort(counts), 321)
    assert a[0] == b[0]             # Gini's integer sum does not depend on the order at all


def test_null_arguments_are_refused(stats):
    lib = capi.lib()
    out = np.zeros(3)
    assert lib.kgx_genotype_statistics(None, 3, 0, capi.ptr(out)) == capi.KGX_EINVAL
    assert b"null" in lib.kgx_last_error()
    one = np.ones(1, dtype=np.uint32)
    assert lib.kgx_genotype_statistics(capi.ptr(one), 1, 0, None) == capi.KGX_EINVAL
