"""kgx_grm_tables / kgx_grm_finish (host only) against the formulas in np.longdouble, and the GRM of the quantised tables against the
long-double GRM within the bound the rounding gives.

The bound: a table entry is t = round(z 2^s), so q = t / 2^s = z + e with |e| <= 2^-(s+1) (e = 0 for code 3, z = 0).  Per row
q_a q_b - z_a z_b = z_a e_b + z_b e_a + e_a e_b, at most (|z_a| + |z_b|) 2^-(s+1) + 4^-(s+1) in magnitude; summed over the m used rows
and divided by m: |G_quantised - G| <= [sum_r (|z_a| + |z_b|) 2^-(s+1) + m 4^-(s+1)] / m.  The integer product is exact; the one
division of kgx_grm_finish adds a relative 2^-53."""
import numpy as np
import pytest

from kgl_gene_amd import capi

LD = np.longdouble
G, MIN_MAF = 60, 0.05


def population():
    rng = np.random.default_rng(5)
    codes = rng.choice(4, size=(48, G), p=[0.55, 0.25, 0.15, 0.05]).astype(np.uint8)
    codes[0], codes[1], codes[2] = 0, 3, 2                     # monomorphic reference, never called, monomorphic alternate
    codes[3] = 0
    codes[3, 7] = 1                                            # p = 1 / 120: below MIN_MAF
    codes[4] = 0
    codes[4, :3], codes[4, 3:5] = 1, 3                         # p = 3 / 116: below MIN_MAF, with no-calls
    counts = np.stack([(codes == c).sum(axis=1) for c in range(4)], axis=1).astype(np.uint32)
    return codes, counts


def reference(counts):
    """(z [n][4] long double, zero where the row is not used; used [n])"""
    c = counts.astype(LD)
    called = c[:, 0] + c[:, 1] + c[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        p = (c[:, 1] + 2 * c[:, 2]) / (2 * called)
        maf = np.minimum(p, 1 - p)
        used = (called > 0) & (maf > 0) & (maf >= LD(MIN_MAF))
        z = (np.arange(3, dtype=LD)[None, :] - 2 * p[:, None]) / np.sqrt(2 * p * (1 - p))[:, None]
    return np.where(used[:, None], np.concatenate([z, np.zeros((len(c), 1), dtype=LD)], axis=1), LD(0)), used


def test_tables_scale_and_used_rows():
    _, counts = population()
    z, used = reference(counts)
    tables, s, rows_used = capi.grm_tables(counts, MIN_MAF)
    assert not used[:5].any() and used[5:].all() and rows_used == used.sum()
    scaled = z * LD(2) ** s
    assert (np.abs(scaled - np.floor(scaled) - LD(0.5)) > 1e-9).all()             # no entry sits at a rounding edge
    assert np.array_equal(tables, np.rint(scaled).astype(np.int16)) and not tables[~used].any()
    assert 0 <= s < 12 and np.abs(tables).max() <= capi.SCORE_MAX < np.abs(np.rint(2 * scaled)).max()      # the largest scale that fits
    assert capi.grm_tables(counts, MIN_MAF, s - 1)[1] == s - 1
    with pytest.raises(capi.KgxError) as refused:
        capi.grm_tables(counts, MIN_MAF, s + 1)
    assert refused.value.code == capi.KGX_EINVAL and "row" in str(refused.value)


def test_finish_is_one_division():
    scores = np.random.default_rng(6).integers(-2 ** 57, 2 ** 57, size=G * (G + 1) // 2)
    got = capi.grm_finish(scores, G, 10, 43)
    want = scores.astype(LD) / LD(43 * 4 ** 10)
    assert (np.abs(got.astype(LD) - want) <= 2 * np.spacing(np.abs(got))).all()
    assert np.isnan(capi.grm_finish(scores, G, 10, 0)).all()


def test_quantised_grm_within_the_rounding_bound():
    codes, counts = population()
    z, used = reference(counts)
    tables, s, m = capi.grm_tables(counts, MIN_MAF)
    rows = np.arange(len(codes))[:, None]
    values = tables.astype(np.int64)[rows, codes]                                 # the reference product of the quantised tables
    a, b = np.triu_indices(G)
    got = capi.grm_finish((values.T @ values)[a, b], G, s, m).astype(LD)
    zg = z[rows, codes]
    want = (zg.T @ zg)[a, b] / LD(m)
    reach = np.abs(zg).sum(axis=0)
    bound = ((reach[a] + reach[b]) * LD(2) ** -(s + 1) + m * LD(4) ** -(s + 1)) / LD(m) + np.abs(want) * LD(2) ** -52
    assert (np.abs(got - want) <= bound).all(), np.max(np.abs(got - want) / bound)
