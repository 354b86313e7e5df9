"""kgx_pair_counts on the device against the plain product: codes [n][G] -> Z = [codes == 1, codes == 2, codes == 3] as int64,
Z Z^T, read at a <= b.  Every word of every pair.

400 rows; G in {37, 65, 200}: one partial 64-genome tile, a diagonal plus an off-diagonal tile pair with a one-genome tail, four
tiles; n_rows in {1, 63, 64, 65, 300}: below, at and past one 64-row step, not a multiple of the 16 rows of an operand's lane."""
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 400


@lru_cache(maxsize=None)
def codes_of(G):
    rng = np.random.default_rng(7000 + G)
    codes = rng.choice(4, size=(V, G), p=[0.6, 0.2, 0.15, 0.05]).astype(np.uint8)
    codes[:, 1] = 2                                            # its own M count is n_rows
    codes[:, 2] = 3                                            # never called
    codes[:, 3] = 0                                            # all reference
    assert len(np.unique(codes[:, G - 1])) == 4                # the last genome of the last tile carries every kind
    return codes


@lru_cache(maxsize=None)
def row_list(n_rows):
    rows = np.random.default_rng(n_rows).permutation(V)[:n_rows].astype(np.uint32)   # shuffled, not adjacent
    if n_rows > 1:
        rows[-1] = rows[0]                                     # ... and one row twice
    return rows


def product(codes):
    G = codes.shape[1]                                                           # -> [G (G + 1) / 2][9] uint32 over the rows of codes [n][G]
    Z = np.stack([codes == 1, codes == 2, codes == 3]).astype(np.int64)          # [kind][row][genome]
    full = np.einsum("pra,qrb->abpq", Z, Z)
    return full[np.triu_indices(G)].reshape(-1, 9).astype(np.uint32)


@lru_cache(maxsize=None)
def expected(G, n_rows, listed):
    return product(codes_of(G)[row_list(n_rows)] if listed else codes_of(G)[:n_rows])


def population(kgx, codes):
    pop = kgx.Population(codes.shape[1], codes.shape[0])
    pop.load_dosage2(kgx.pack_dosage2(codes))
    return pop


def assert_same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("G", [37, 65, 200])
def test_every_word_equals_the_product(kgx, G, n_rows, listed):
    codes = codes_of(G)
    pop = population(kgx, codes)
    rows = row_list(n_rows) if listed else None
    got = pop.pair_counts(rows, n_rows)
    pop.close()
    assert_same(got, expected(G, n_rows, listed))
    own = got[[kgx.pair_index(g, g, G) for g in (1, 2, 3)]]
    assert own[0].tolist() == [0, 0, 0, 0, n_rows, 0, 0, 0, 0] and own[1].tolist() == [0] * 8 + [n_rows] and not own[2].any()


def test_genome_mask(kgx):
    G = 200
    codes = codes_of(G)
    keep = (np.arange(G) % 7 != 0).astype(np.uint8)
    pop = population(kgx, codes)
    pop.set_genome_mask(keep)
    got = pop.pair_counts()
    by_genome = pop.count_by_genome()
    pop.close()
    assert_same(got, product(codes * keep))
    left_out = [kgx.pair_index(min(a, b), max(a, b), G) for a in range(0, G, 7) for b in range(G)]
    assert not got[left_out].any()
    diagonal = got[[kgx.pair_index(g, g, G) for g in range(G)]]
    assert np.array_equal(diagonal[:, [0, 4, 8]][keep != 0], by_genome[:, 1:4][keep != 0])


@pytest.fixture
def rebind(kgx):
    yield kgx.init
    kgx.init(0)


def test_one_device_listed_three_times(kgx, rebind):
    G = 200
    rebind([0, 0, 0])
    pop = population(kgx, codes_of(G))
    assert len([s for s in pop.shards if s["n_genomes"]]) == 3
    got = pop.pair_counts(row_list(300))
    pop.close()
    assert_same(got, expected(G, 300, True))


@pytest.mark.parametrize("switch,value,batches,splits", [("KGX_PAIRS_ROWS", "300", 1, 5), ("KGX_PAIRS_ROWS", "64", 5, 1), ("KGX_PAIRS_ROWS", "7", 43, 1),
                                                        ("KGX_PAIRS_SPLITS", "1", 1, 1), ("KGX_PAIRS_SPLITS", "2", 1, 2)])
def test_row_batches_and_slices_change_nothing(kgx, monkeypatch, switch, value, batches, splits):
    """Batches of one step store, then add (43 batches of 7 rows); KGX_PAIRS_SPLITS=1 walks the five steps in one workgroup, =2
    as three and two."""
    G = 200
    pop = population(kgx, codes_of(G))
    monkeypatch.setenv(switch, value)
    kgx.reload_options()
    try:
        got = pop.pair_counts(row_list(300))
        ms, reported_batches, reported_splits = kgx.pair_counts_last()
    finally:
        monkeypatch.delenv(switch)
        kgx.reload_options()
        pop.close()
    assert (reported_batches, reported_splits) == (batches, splits) and ms > 0.0
    assert_same(got, expected(G, 300, True))


def test_one_tile_pair_splits_its_rows(kgx):
    G = 37
    pop = population(kgx, codes_of(G))
    got = pop.pair_counts(n_rows=300)
    _, batches, splits = kgx.pair_counts_last()
    pop.close()
    assert batches == 1 and splits == 5                        # one tile pair: a slice per 64-row step
    assert_same(got, expected(G, 300, False))


def test_refusals(kgx):
    G = 37
    pop = population(kgx, codes_of(G))
    out = np.zeros((G * (G + 1) // 2, 9), dtype=np.uint32)
    rows = np.array([5, V], dtype=np.uint32)
    assert kgx.lib().kgx_pair_counts(pop._h, kgx.ptr(rows), 2, kgx.ptr(out)) == kgx.KGX_EINVAL
    assert "rows[1]" in kgx.lib().kgx_last_error().decode()
    assert kgx.lib().kgx_pair_counts(pop._h, None, V + 1, kgx.ptr(out)) == kgx.KGX_EINVAL
    assert kgx.lib().kgx_pair_counts(pop._h, None, V, None) == kgx.KGX_EINVAL
    out[:] = 1
    assert kgx.lib().kgx_pair_counts(pop._h, None, 0, kgx.ptr(out)) == kgx.KGX_OK and not out.any()
    pop.close()
