"""kgx_pair_scores on the device against the plain product in int64: V = tables[i][codes[i][g]] ([n][G]), V^T V, read at a <= b.
Every word, by equality.  Populations and row lists as in test_pair_counts_gpu.py; the tables are random int16 within +-SCORE_MAX
with the four extreme rows (every code at +-8128, +-8127) first."""
from functools import lru_cache

import numpy as np
import pytest

from kgl_gene_amd.capi import SCORE_ACC_ROWS, SCORE_MAX

pytestmark = pytest.mark.gpu

V = 400


@lru_cache(maxsize=None)
def codes_of(G):
    rng = np.random.default_rng(7000 + G)
    codes = rng.choice(4, size=(V, G), p=[0.6, 0.2, 0.15, 0.05]).astype(np.uint8)
    codes[:, 1], codes[:, 2], codes[:, 3] = 2, 3, 0           # all M, never called, all reference
    return codes


@lru_cache(maxsize=None)
def row_list(n_rows):
    rows = np.random.default_rng(n_rows).permutation(V)[:n_rows].astype(np.uint32)   # shuffled, not adjacent
    if n_rows > 1:
        rows[-1] = rows[0]                                     # ... and one row twice
    return rows


@lru_cache(maxsize=None)
def tables_of(n_rows):
    tables = np.random.default_rng(90 + n_rows).integers(-SCORE_MAX, SCORE_MAX + 1, size=(n_rows, 4)).astype(np.int16)
    extremes = np.array([SCORE_MAX, -SCORE_MAX, SCORE_MAX - 1, 1 - SCORE_MAX], dtype=np.int16)[:n_rows]
    tables[:len(extremes)] = extremes[:, None]
    return tables


def product(codes, tables, dtype=np.int64):
    values = tables.astype(dtype)[np.arange(len(codes))[:, None], codes]          # [n][G]
    return (values.T @ values)[np.triu_indices(codes.shape[1])]


@lru_cache(maxsize=None)
def expected(G, n_rows, listed):
    return product(codes_of(G)[row_list(n_rows)] if listed else codes_of(G)[:n_rows], tables_of(n_rows))


def population(kgx, codes):
    pop = kgx.Population(codes.shape[1], codes.shape[0])
    pop.load_dosage2(kgx.pack_dosage2(codes))
    return pop


def assert_same(got, want):
    assert got.shape == want.shape and got.dtype == np.int64
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("G", [37, 65, 200])
def test_every_score_equals_the_product(kgx, G, n_rows, listed):
    pop = population(kgx, codes_of(G))
    got = pop.pair_scores(tables_of(n_rows), row_list(n_rows) if listed else None, n_rows)
    pop.close()
    assert_same(got, expected(G, n_rows, listed))


def test_one_hot_tables_are_the_pair_counts(kgx):
    G, rows = 200, row_list(300)
    pop = population(kgx, codes_of(G))
    counts = pop.pair_counts(rows).astype(np.int64)
    got = [pop.pair_scores(np.tile(np.array(t, dtype=np.int16), (300, 1)), rows) for t in ((0, 1, 0, 0), (0, 0, 1, 0), (1, 1, 1, 0))]
    pop.close()
    own = counts[[kgx.pair_index(g, g, G) for g in range(G)], 8]                  # no-calls per genome
    a, b = np.triu_indices(G)
    assert_same(got[0], counts[:, 0])
    assert_same(got[1], counts[:, 4])
    assert_same(got[2], 300 - own[a] - own[b] + counts[:, 8])                     # the jointly called rows


def test_genome_mask(kgx):
    G = 200
    keep = (np.arange(G) % 7 != 0).astype(np.uint8)
    pop = population(kgx, codes_of(G))
    pop.set_genome_mask(keep)
    got = pop.pair_scores(tables_of(V))                                            # the code-0 entries are not 0
    pop.close()
    a, b = np.triu_indices(G)
    want = np.where((keep[a] & keep[b]) != 0, expected(G, V, False), 0)
    assert want[kgx.pair_index(1, 3, G)] != 0 and not want[kgx.pair_index(0, 0, G)]
    assert_same(got, want)


@pytest.fixture
def rebind(kgx):
    yield kgx.init
    kgx.init(0)


def test_one_device_listed_three_times(kgx, rebind):
    G = 200
    rebind([0, 0, 0])
    pop = population(kgx, codes_of(G))
    assert len([s for s in pop.shards if s["n_genomes"]]) == 3
    got = pop.pair_scores(tables_of(300), row_list(300))
    pop.close()
    assert_same(got, expected(G, 300, True))


@pytest.mark.parametrize("G,switch,value,batches,splits", [(200, "KGX_SCORES_ROWS", "64", 5, 1), (200, "KGX_SCORES_ROWS", "448", 1, 5), (200, None, None, 1, 5),
                                                          (37, "KGX_SCORES_SPLITS", "1", 1, 1), (37, "KGX_SCORES_SPLITS", "2", 1, 2),
                                                          (37, "KGX_SCORES_SPLITS", "5", 1, 5)])
def test_row_batches_and_slices_change_nothing(kgx, monkeypatch, G, switch, value, batches, splits):
    """Batches of one step store, then add; KGX_SCORES_SPLITS=1 walks the five steps in one workgroup, =2 as three and two."""
    pop = population(kgx, codes_of(G))
    if switch:
        monkeypatch.setenv(switch, value)
    got = pop.pair_scores(tables_of(300), row_list(300))
    ms, reported_batches, reported_splits = kgx.pair_scores_last()
    pop.close()
    assert (reported_batches, reported_splits) == (batches, splits) and ms > 0.0
    assert_same(got, expected(G, 300, True))


def test_accumulation_bound(kgx, monkeypatch):
    """More rows than one int32 accumulation may take, in ONE slice: the call has to cut them into two launches.  Both digits of
    +-8128 are at their largest; the float64 product is exact, |S| <= 2^26 n < 2^53."""
    G, n = 65, SCORE_ACC_ROWS + 65
    assert 2 ** 26 * n < 2 ** 53
    rng = np.random.default_rng(17)
    rows = rng.integers(0, V, size=n).astype(np.uint32)
    tables = rng.choice(np.array([SCORE_MAX, -SCORE_MAX], dtype=np.int16), size=(n, 4))
    pop = population(kgx, codes_of(G))
    monkeypatch.setenv("KGX_SCORES_SPLITS", "1")
    got = pop.pair_scores(tables, rows)
    _, batches, splits = kgx.pair_scores_last()
    pop.close()
    assert (batches, splits) == (2, 1)
    assert_same(got, product(codes_of(G)[rows], tables, np.float64).astype(np.int64))


def test_refusals(kgx):
    G = 37
    pop = population(kgx, codes_of(G))
    call, out = kgx.lib().kgx_pair_scores, np.ones(G * (G + 1) // 2, dtype=np.int64)
    tables = tables_of(2).copy()
    assert call(pop._h, kgx.ptr(np.array([5, V], dtype=np.uint32)), 2, kgx.ptr(tables), kgx.ptr(out)) == kgx.KGX_EINVAL
    assert "rows[1]" in kgx.lib().kgx_last_error().decode()
    assert call(pop._h, None, 2, None, kgx.ptr(out)) == kgx.KGX_EINVAL
    tables[1, 2] = SCORE_MAX + 1
    assert call(pop._h, None, 2, kgx.ptr(tables), kgx.ptr(out)) == kgx.KGX_EINVAL
    assert "tables[1][2]" in kgx.lib().kgx_last_error().decode()
    assert call(pop._h, None, 0, kgx.ptr(tables), kgx.ptr(out)) == kgx.KGX_OK and not out.any()
    pop.close()
