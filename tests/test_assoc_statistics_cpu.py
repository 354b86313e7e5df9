"""kgx_assoc_columns and kgx_assoc_statistics (host only).  The columns against np.rint bit for bit; the scan against a plain
per-row long-double least-squares fit of q / 2^s on the dosage over the called, kept genomes.  The sums are the plain product the
device test compares kgx_column_sums with, so this runs without a GPU.

beta is two integer-to-double conversions and one division (1.5 x 2^-53 from the exact quotient): the bound of
test_ld_statistics_cpu.py, 1e-14.  t is two conversions, two square roots, a division and a multiplication of exact integers: the
largest relative error against the long-double fit on these inputs is 2.56e-16 (beta: 1.39e-16); the bound is 16 times that."""
import numpy as np
import pytest

from kgl_gene_amd import capi

G, N_ROWS, TRAITS = 200, 50, 3
BETA_RTOL, T_RTOL = 1e-14, 16 * 2.56e-16
RNG = np.random.default_rng(2024)
CODES = RNG.choice(4, size=(N_ROWS, G), p=[0.45, 0.3, 0.2, 0.05]).astype(np.uint8)
KEEP = (np.arange(G) % 7 != 0).astype(np.uint8)
Y = np.stack([RNG.normal(size=G), 0.4 * np.minimum(CODES[10], 2) + RNG.normal(size=G), RNG.uniform(-3.0, 5.0, size=G)])


def sums_of(codes, columns, keep):
    Z = np.stack([codes == 1, codes == 2, codes == 3]).astype(np.int64)
    return np.einsum("kig,jg->ijk", Z, columns.astype(np.int64) * keep)


def counts_of(codes, keep):
    return np.stack([((codes == c) & (keep != 0)).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32)


def scan(codes, columns, bits, keep):
    return capi.assoc_statistics(sums_of(codes, columns, keep), counts_of(codes, keep), columns, bits, keep)


def test_columns_are_rint_at_the_largest_scale_that_fits():
    columns, bits = capi.assoc_columns(Y)
    q = np.rint(np.ldexp(Y, bits)).astype(np.int64)
    assert columns.dtype == np.int32 and np.array_equal(columns, np.concatenate([q, q * q]))
    assert np.abs(q).max() <= 8128 < np.abs(np.rint(np.ldexp(Y, bits + 1))).max() and bits < 12
    assert capi.assoc_columns(Y / 64.0)[1] == 12               # never above 12
    edge = np.array([[8128.5, -8128.5, 0.5, 1.5]])             # to nearest even: 8128 fits at s = 0
    assert np.array_equal(capi.assoc_columns(edge)[0][0], [8128, -8128, 0, 2]) and capi.assoc_columns(edge)[1] == 0
    given, used = capi.assoc_columns(Y, 3)
    assert used == 3 and np.array_equal(given[:TRAITS], np.rint(Y * 8.0).astype(np.int32))


@pytest.mark.parametrize("y,bits,needle", [([[0.0, 1.0], [2.0, np.nan]], -1, "y[1][1]"), ([[0.0, np.inf]], 2, "y[0][1]"), ([[1.0, -8129.0]], -1, "y[0][1]"),
                                           ([[3.0, 2033.0]], 2, "y[0][1]"), ([[1.0]], 13, "above 12")])
def test_columns_refusals(y, bits, needle):
    with pytest.raises(capi.KgxError) as e:
        capi.assoc_columns(np.array(y), bits)
    assert e.value.code == capi.KGX_EINVAL and needle in str(e.value)


def test_scan_against_the_long_double_fit():
    columns, bits = capi.assoc_columns(Y)
    beta, t = scan(CODES, columns, bits, KEEP)
    worst = [0.0, 0.0]
    for i in range(N_ROWS):
        used = (CODES[i] != 3) & (KEEP != 0)
        x = CODES[i][used].astype(np.longdouble)
        for k in range(TRAITS):
            y = columns[k][used].astype(np.longdouble) / np.longdouble(2**bits)
            dx, dy = x - x.mean(), y - y.mean()
            slope = (dx * dy).sum() / (dx * dx).sum()
            rest = dy - slope * dx
            want_t = slope / np.sqrt((rest * rest).sum() / (len(x) - 2) / (dx * dx).sum())
            assert abs((dx * dy).sum() / np.sqrt((dx * dx).sum() * (dy * dy).sum())) <= 0.95          # the reference is well conditioned
            errors = [abs(beta[i, k] - slope) / abs(slope), abs(t[i, k] - want_t) / abs(want_t)]
            worst = [max(float(a), float(b)) for a, b in zip(worst, errors)]
            assert errors[0] <= BETA_RTOL and errors[1] <= T_RTOL, (i, k, beta[i, k], slope, t[i, k], want_t)
    print("largest relative error: beta %.3g, t %.3g" % tuple(worst))


def test_undefined_and_fixed_values():
    codes = CODES[:5].copy()
    codes[0] = 3
    codes[0, 1:3] = [0, 1]                                     # two called genomes: N < 3
    codes[1] = np.where(codes[1] == 3, 3, 2)                   # monomorphic
    codes[4] = np.where(codes[4] == 3, 0, codes[4])            # every genome called
    y = np.stack([Y[0], np.full(G, 1.25), codes[4].astype(np.float64), -codes[4].astype(np.float64)])   # noise, a constant, the dosage of row 4, its negative
    columns, bits = capi.assoc_columns(y)
    beta, t = scan(codes, columns, bits, np.ones(G, dtype=np.uint8))
    assert np.isnan(beta[0]).all() and np.isnan(t[0]).all() and np.isnan(beta[1]).all() and np.isnan(t[1]).all()
    assert np.isnan(beta[:, 1]).all() and np.isnan(t[:, 1]).all()
    assert np.isfinite(beta[2:, 0]).all() and np.isfinite(t[2:, 0]).all()
    assert beta[4, 2] == 1.0 and t[4, 2] == np.inf and beta[4, 3] == -1.0 and t[4, 3] == -np.inf
