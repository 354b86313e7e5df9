"""The allele census' host side, without a device: the NumPy restatement (tests/allele_census_reference.py) against a per-cell
Python loop, and kgx_census_allele_frequencies against float32(float64(AC) / float64(AN)), bit for bit."""
import numpy as np
import pytest

from tests import allele_census_reference as acr


def loop_census(cells, groups, n_groups, amax):
    """kgx.h's description of the census, one cell at a time."""
    L, G = cells.shape
    out = np.zeros((L, n_groups, 3 + 2 * amax), dtype=np.uint32)
    for l in range(L):
        for g in range(G):
            if groups[g] == 0xFF:
                continue
            words = out[l, groups[g]]
            byte = int(cells[l, g])
            if byte == 0x00:
                words[0] += 1
            if byte == 0xFF:
                words[2] += 1
                continue
            lo, hi = byte & 15, byte >> 4
            if hi == 0:
                copies = [lo]
            elif lo == 0:
                copies = [hi, hi]
            else:
                copies = [lo, hi]
            copies = [x for x in copies if x != 0]
            for a in set(copies):
                n = copies.count(a)
                if a == 15 or a > amax:
                    words[1] += n
                else:
                    words[3 + 2 * (a - 1) + (n - 1)] += 1
    return out


def special_case():
    """7 loci x 23 genomes holding every special cell: (a,0), (a,a), (0,a), (a,b), (15,0), (a,15), (15,a), (0,15), 0xFF (which is also
    (15,15)), an index past amax, a locus crowded throughout, a locus where everybody holds (a,a), a group without a genome, genomes
    in no group."""
    def cell(lo, hi):
        return lo | (hi << 4)
    L, G = 7, 23
    cells = np.zeros((L, G), dtype=np.uint8)
    cells[0, :9] = [cell(1, 0), cell(1, 1), cell(0, 1), cell(1, 2), cell(2, 1), cell(15, 0), cell(1, 15), cell(15, 1), cell(0, 15)]
    cells[0, 9:14] = [0xFF, cell(5, 0), cell(0, 5), cell(5, 5), cell(3, 5)]
    cells[1] = 0xFF
    cells[2] = cell(2, 2)
    cells[3, ::2] = cell(3, 0)
    cells[3, 1::4] = cell(0, 3)
    cells[4, 20:] = [cell(14, 14), cell(14, 0), cell(13, 14)]
    cells[6, 22] = cell(2, 3)                                   # locus 5 stays all reference
    groups = (np.arange(G) % 4).astype(np.uint8)
    groups[groups == 2] = 4                                     # group 2 has no genome
    groups[[5, 17]] = 0xFF                                      # in no group
    return cells, groups


@pytest.mark.parametrize("amax", [1, 3, 14])
def test_restatement_equals_the_cell_loop(amax):
    cells, groups = special_case()
    want = loop_census(cells, groups, 6, amax)
    got = acr.census(cells, groups, 6, amax)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert not got[:, 2].any() and not got[:, 5].any()          # the groups without a genome
    assert got[1, :, 2].sum() == 21 and got[1, :, [0, 1] + list(range(3, 3 + 2 * amax))].sum() == 0      # crowded throughout: nothing else counted
    if amax >= 2:
        assert got[2, :, 4 + 2].sum() == 21 and got[2, :, 3 + 2].sum() == 0


def test_restatement_on_random_cells_equals_the_cell_loop():
    rng = np.random.default_rng(5)
    cells = rng.integers(0, 256, (40, 31), dtype=np.uint8)
    groups = rng.choice([0, 1, 2, 0xFF], 31).astype(np.uint8)
    for amax in (2, 7):
        assert np.array_equal(acr.census(cells, groups, 3, amax), loop_census(cells, groups, 3, amax))


@pytest.mark.parametrize("amax", [1, 3, 14])
def test_copies_identity_on_random_censuses(amax):
    """sum over a of (single_a + 2 double_a) + unknown_copies = the copies the restatement counts cell by cell."""
    rng = np.random.default_rng(amax)
    cells = rng.integers(0, 256, (200, 57), dtype=np.uint8)
    cells[rng.random(cells.shape) < 0.5] = 0
    groups = rng.choice([0, 1, 2, 3, 0xFF], 57).astype(np.uint8)
    words = acr.census(cells, groups, 4, amax).astype(np.int64)
    counted = (words[:, :, 3::2] + 2 * words[:, :, 4::2]).sum(-1) + words[:, :, 1]
    copies = acr.cell_copies(cells).sum(-1, dtype=np.int64)     # [L][G]: every copy of every cell
    for g in range(4):
        assert np.array_equal(counted[:, g], copies[:, groups == g].sum(1))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def frequency_case(amax=3, n_groups=6):
    rng = np.random.default_rng(77)
    L = 300
    sizes = np.array([11, 7, 0, 5, 9, 3], dtype=np.uint64)[:n_groups]
    words = np.zeros((L, n_groups, 3 + 2 * amax), dtype=np.uint32)
    for g in range(n_groups):
        for a in range(amax):
            single = rng.integers(0, int(sizes[g]) + 1, L)
            double = rng.integers(0, int(sizes[g]) + 1, L)
            double = np.minimum(double, int(sizes[g]) - single)
            words[:, g, 3 + 2 * a], words[:, g, 4 + 2 * a] = single, double
    words[:, :, 1] = rng.integers(0, 5, (L, n_groups))          # unknown copies: must never enter
    words[0, :, 3:] = 0                                          # AC = 0 everywhere
    words[1, :, 3:] = 0
    words[1, :, 4] = sizes.astype(np.uint32)                     # AC = AN for alt 1: everybody holds it twice
    n_alt = rng.integers(0, amax + 1, L).astype(np.uint8)
    n_alt[:2] = amax
    return words, sizes, n_alt


def expected_frequencies(words, sizes, pool, n_alt):
    """np.float32(np.float64(AC) / np.float64(AN)).astype(np.float64), written out here independently of the restatement module."""
    L, _, k = words.shape
    amax = (k - 3) // 2
    out = np.full((L, amax), np.nan)
    an = 2 * sum(int(sizes[p]) for p in pool)
    if an == 0:
        return out
    for l in range(L):
        for a in range(amax if n_alt is None else min(int(n_alt[l]), amax)):
            ac = sum(int(words[l, p, 3 + 2 * a]) + 2 * int(words[l, p, 4 + 2 * a]) for p in pool)
            out[l, a] = np.float32(np.float64(ac) / np.float64(an)).astype(np.float64)
    return out


@pytest.mark.parametrize("pool", [[0], [1], [4], [5], [0, 1, 2, 3, 4, 5], [3, 0], [2], []], ids=str)
@pytest.mark.parametrize("with_n_alt", [True, False])
def test_census_allele_frequencies_bit_for_bit(pool, with_n_alt):
    from kgl_gene_amd import capi

    capi.ensure_built()
    words, sizes, n_alt = frequency_case()
    alts = n_alt if with_n_alt else None
    got = capi.census_allele_frequencies(words, sizes, pool, alts)
    want = expected_frequencies(words, sizes, pool, alts)
    assert got.shape == want.shape == (300, 3)
    assert np.array_equal(np.isnan(got), np.isnan(want))         # NaNs by position
    assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])
    assert np.array_equal(bits(acr.allele_frequencies(words, sizes, pool, alts))[~np.isnan(want)], bits(want)[~np.isnan(want)])
    empty = sum(int(sizes[p]) for p in pool) == 0
    if empty:                                                    # an empty pool, a pool of a group without genomes: AN == 0
        assert np.isnan(got).all()
    else:
        assert (got[0] == 0.0).all() and not np.signbit(got[0]).any()   # AC == 0: 0.0, not NaN
        if pool == [0, 1, 2, 3, 4, 5] or len(pool) == 1:
            assert got[1, 0] == 1.0                               # AC == AN
        if with_n_alt:
            assert np.isnan(got[np.arange(3)[None, :] >= n_alt[:, None]]).all()


def test_census_allele_frequencies_refuses_bad_arguments():
    from kgl_gene_amd import capi

    capi.ensure_built()
    words, sizes, _ = frequency_case()
    with pytest.raises(capi.KgxError) as e:
        capi.census_allele_frequencies(words, sizes, [6])
    assert e.value.code == capi.KGX_EINVAL and "pool" in str(e.value)
    out = np.zeros((300, 3))
    lib = capi.lib()
    assert lib.kgx_census_allele_frequencies(capi.ptr(words), 300, 6, 3, None, None, 0, None, capi.ptr(out)) == capi.KGX_EINVAL
    assert lib.kgx_census_allele_frequencies(capi.ptr(words), 300, 6, 15, capi.ptr(sizes), None, 0, None, capi.ptr(out)) == capi.KGX_EINVAL
    assert lib.kgx_census_allele_frequencies(capi.ptr(words), 300, 33, 3, capi.ptr(sizes), None, 0, None, capi.ptr(out)) == capi.KGX_EINVAL
