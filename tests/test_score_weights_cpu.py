"""kgx_score_weights and kgx_score_finish (host only).  The weights against np.rint bit for bit; the scores against a plain
long-double evaluation of sum of quantised weight x dosage with the imputed term.  The sums are the plain product the device test
compares kgx_genome_scores with, so this runs without a GPU.

The finish is one int64-to-double conversion (one rounding, 2^-53 relative) and an exact scaling: the bound is 2^-52, derived and
not measured, and where |sum| < 2^53 the conversion is exact and the test asserts equality."""
import numpy as np
import pytest

from kgl_gene_amd import capi

G, N_ROWS, SCORES = 50, 200, 2
RNG = np.random.default_rng(2025)
CODES = RNG.choice(4, size=(N_ROWS, G), p=[0.45, 0.3, 0.2, 0.05]).astype(np.uint8)
CODES[7] = 3                                                   # a row nobody is called in
COUNTS = np.stack([(CODES == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32)
BETA = RNG.normal(scale=3.0, size=(SCORES, N_ROWS))          # the largest scale that fits is below the cap of 12
CALLED = COUNTS[:, :3].sum(axis=1)
TWICE_P = np.divide((COUNTS[:, 1] + 2.0 * COUNTS[:, 2]), CALLED, out=np.zeros(N_ROWS), where=CALLED > 0)


def test_weights_are_rint_at_the_largest_scale_that_fits():
    weights, bits = capi.score_weights(BETA, COUNTS)
    assert weights.dtype == np.int16 and weights.shape == (2 * SCORES, N_ROWS) and not weights[SCORES:, 7].any()
    assert np.array_equal(weights, np.concatenate([np.rint(BETA * 2.0**bits), np.rint(TWICE_P * BETA * 2.0**bits)]))
    larger = np.concatenate([np.rint(BETA * 2.0**(bits + 1)), np.rint(TWICE_P * BETA * 2.0**(bits + 1))])
    assert np.abs(weights).max() <= 8128 < np.abs(larger).max() and bits < 12
    assert capi.score_weights(BETA / 64.0)[1] == 12            # never above 12
    given, used = capi.score_weights(BETA, None, 3)
    assert used == 3 and given.shape == (SCORES, N_ROWS) and np.array_equal(given, np.rint(BETA * 8.0))


@pytest.mark.parametrize("beta,bits,needle", [([[0.0, 1.0], [np.nan, 2.0]], -1, "beta[1][0]"), ([[0.0, np.inf]], 2, "beta[0][1]"), ([[3.0, 2033.0]], 2, "beta[0][1]"),
                                              ([[1.0, -8129.0]], -1, "beta[0][1]"), ([[1.0]], 13, "above 12")])
def test_weights_refusals(beta, bits, needle):
    with pytest.raises(capi.KgxError) as e:
        capi.score_weights(np.array(beta), None, bits)
    assert e.value.code == capi.KGX_EINVAL and needle in str(e.value)


@pytest.mark.parametrize("shift", [0, 56])
def test_scores_against_the_long_double_sum(shift):
    """shift 56 puts 2^56 + 1 onto every S_H: sums past 2^53, where the conversion rounds."""
    weights, bits = capi.score_weights(BETA, COUNTS)
    q, m = weights[:SCORES].astype(np.int64), weights[SCORES:].astype(np.int64)
    Z = np.stack([CODES == 1, CODES == 2, CODES == 3]).astype(np.int64)
    sums = np.einsum("kig,ji->gjk", Z, weights.astype(np.int64))
    sums[:, :SCORES, 0] += ((1 << shift) + 1) if shift else 0
    got = capi.score_finish(sums, SCORES, bits, imputed=True)
    plain = capi.score_finish(sums[:, :SCORES], SCORES, bits)
    dosage, missing = np.minimum(CODES, 2) * (CODES != 3), (CODES == 3)
    for g in range(G):
        for j in range(SCORES):
            called = int((q[j] * dosage[:, g]).sum()) + (((1 << shift) + 1) if shift else 0)
            imputed = called + int((m[j] * missing[:, g]).sum())
            for value, whole in ((got[g, j], imputed), (plain[g, j], called)):
                want = (np.longdouble(whole >> 32) * np.longdouble(2**32) + np.longdouble(whole & 0xFFFFFFFF)) / np.longdouble(2**bits)   # exact: below 2^64
                assert abs(np.longdouble(value) - want) <= np.longdouble(2.0**-52) * abs(want), (g, j, value, want)
                if abs(whole) < 2**53:
                    assert np.longdouble(value) == want, (g, j, value, want)
