"""kgx_column_sums on the device against the plain product: codes [n][G] -> Z = [codes == 1, codes == 2, codes == 3] as int64,
einsum with the int64 columns.  Every word.

400 rows with the code distribution and special rows of test_ld_counts_gpu.py; G in {37, 65, 600, 2100}: one partial chunk; a
one-genome tail chunk; pitch 160 = 10 chunks = 2 1/2 segments, the last segment's upper chunks must not be read; 33 chunks, 9
segments, split.  n_rows below, at and past one 64-row block.  n_columns 1, 16, 17, 40: a partial group, one group, a group and one
column, three groups of four digits = 12 tiles = a second pass of tiles."""
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 400
MAX = 1 << 26
EDGES = [0, 63, 64, 65, 8127, 8128, 8192, 1048575, 1048576, MAX]


@lru_cache(maxsize=None)
def codes_of(G):
    rng = np.random.default_rng(9000 + G)
    codes = rng.choice(4, size=(V, G), p=[0.6, 0.2, 0.15, 0.05]).astype(np.uint8)
    codes[1], codes[2], codes[3] = 2, 3, 0                     # all minor homozygous, never called, all reference
    codes[4:8, G - 1] = [0, 1, 2, 3]                           # the last genome of the last chunk carries every kind
    return codes


@lru_cache(maxsize=None)
def columns_of(G, C, mixed=False):
    rng = np.random.default_rng(77 * G + C)
    cols = rng.integers(-MAX, MAX + 1, size=(C, G)).astype(np.int32)
    planted = np.array([s * e for e in EDGES for s in (1, -1)], dtype=np.int32)
    at = rng.permutation(C * (G - 1))[:len(planted)]           # the digit edges, anywhere but the last genome
    cols[at // (G - 1), at % (G - 1)] = planted
    cols[:, G - 1] = np.where(np.arange(C) % 2, -MAX, MAX)
    if mixed:                                                  # groups of one, two and four digits
        cols[:16] = rng.integers(-63, 64, size=(16, G))
        cols[16:32] = rng.integers(-8128, 8129, size=(16, G))
    return cols


@lru_cache(maxsize=None)
def row_list(n_rows):
    rows = np.random.default_rng(n_rows).permutation(V)[:n_rows].astype(np.uint32)   # shuffled, not adjacent
    if n_rows > 1:
        rows[-1] = rows[0]                                     # ... and one row twice
    return rows


def product(codes, columns):
    Z = np.stack([codes == 1, codes == 2, codes == 3]).astype(np.int64)
    return np.einsum("kig,jg->ijk", Z, columns.astype(np.int64))


@lru_cache(maxsize=None)
def expected(G, C, mixed=False):
    return product(codes_of(G), columns_of(G, C, mixed))       # of all 400 rows, once


def population(kgx, codes):
    pop = kgx.Population(codes.shape[1], codes.shape[0])
    pop.load_dosage2(kgx.pack_dosage2(codes))
    return pop


def assert_same(got, want):
    assert got.shape == want.shape and got.dtype == np.int64
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("C", [1, 16, 17, 40])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("G", [37, 65, 600, 2100])
def test_every_word_equals_the_product(kgx, G, n_rows, C, listed):
    pop = population(kgx, codes_of(G))
    got = pop.column_sums(columns_of(G, C), row_list(n_rows) if listed else None, n_rows)
    pop.close()
    assert_same(got, expected(G, C)[row_list(n_rows) if listed else slice(n_rows)])


def test_groups_of_one_two_and_four_digits(kgx):
    G, C = 600, 40
    pop = population(kgx, codes_of(G))
    got = pop.column_sums(columns_of(G, C, True), row_list(200))
    pop.close()
    assert_same(got, expected(G, C, True)[row_list(200)])


def test_genome_mask(kgx):
    G, C = 600, 17
    keep = (np.arange(G) % 7 != 0).astype(np.uint8)
    columns = columns_of(G, C).copy()
    columns[3] = 1
    pop = population(kgx, codes_of(G))
    pop.set_genome_mask(keep)
    got = pop.column_sums(columns)
    by_locus = pop.allele_count_by_locus()
    pop.close()
    assert_same(got, product(codes_of(G), columns * keep))
    assert np.array_equal(got[:, 3], by_locus[:, 1:4])


@pytest.fixture
def rebind(kgx):
    yield kgx.init
    kgx.init(0)


def test_one_device_listed_three_times(kgx, rebind):
    G, C = 600, 40
    rebind([0, 0, 0])
    pop = population(kgx, codes_of(G))
    assert len([s for s in pop.shards if s["n_genomes"]]) == 3
    got = pop.column_sums(columns_of(G, C), row_list(200))
    pop.close()
    assert_same(got, expected(G, C)[row_list(200)])


@pytest.mark.parametrize("switch,value,batches,splits", [("KGX_ASSOC_ROWS", "64", 4, 9), ("KGX_ASSOC_ROWS", "7", 4, 9), ("KGX_ASSOC_SPLITS", "1", 1, 1),
                                                        ("KGX_ASSOC_SPLITS", "2", 1, 2)])
def test_batches_and_slices_change_nothing(kgx, monkeypatch, switch, value, batches, splits):
    """G = 2100 is nine 256-genome segments; 200 rows are four blocks and 17 full-range columns one pass: without a cap a slice per
    segment.  A cap of 7 rows is one block a batch; KGX_ASSOC_SPLITS=1 walks the nine segments in one workgroup and stores plainly,
    =2 as five and four."""
    G, C = 2100, 17
    pop = population(kgx, codes_of(G))
    monkeypatch.setenv(switch, value)
    kgx.reload_options()
    try:
        got = pop.column_sums(columns_of(G, C), row_list(200))
        ms, reported_batches, reported_splits = kgx.column_sums_last()
    finally:
        monkeypatch.delenv(switch)
        kgx.reload_options()
        pop.close()
    assert (reported_batches, reported_splits) == (batches, splits) and ms > 0.0
    assert_same(got, expected(G, C)[row_list(200)])


@pytest.mark.parametrize("case,needle", [("value", "columns[2][5]"), ("negative", "columns[0][36]"), ("row", "rows[1]"), ("n_rows", "n_rows"),
                                         ("no columns", "no columns"), ("pop", "null"), ("out", "null"), ("columns", "null"), ("overflow", "overflow"),
                                         ("shard", "2^25")])
def test_refusals(kgx, case, needle):
    G = 37
    pop = kgx.Population((1 << 25) + 1, 1) if case == "shard" else population(kgx, codes_of(G))
    columns = np.zeros((3, (1 << 25) + 1), dtype=np.int32) if case == "shard" else columns_of(G, 3).copy()
    out = np.ones((V, 3, 3), dtype=np.int64)
    rows = np.array([5, V if case == "row" else 6], dtype=np.uint32)
    if case == "value":
        columns[2, 5] = MAX + 1
    if case == "negative":
        columns[0, 36] = -MAX - 1
    args = {"n_rows": (pop._h, None, V + 1, kgx.ptr(columns), 3, kgx.ptr(out)), "no columns": (pop._h, None, V, kgx.ptr(columns), 0, kgx.ptr(out)),
            "pop": (None, None, V, kgx.ptr(columns), 3, kgx.ptr(out)), "out": (pop._h, None, V, kgx.ptr(columns), 3, None),
            "columns": (pop._h, None, V, None, 3, kgx.ptr(out)), "overflow": (pop._h, kgx.ptr(rows), 1 << 61, kgx.ptr(columns), 3, kgx.ptr(out)), "shard": (pop._h, None, 1, kgx.ptr(columns), 3, kgx.ptr(out))}
    assert kgx.lib().kgx_column_sums(*args.get(case, (pop._h, kgx.ptr(rows), 2, kgx.ptr(columns), 3, kgx.ptr(out)))) == kgx.KGX_EINVAL
    assert needle in kgx.lib().kgx_last_error().decode()
    assert kgx.lib().kgx_column_sums(pop._h, None, 0, kgx.ptr(columns), 3, kgx.ptr(out)) == kgx.KGX_OK      # n_rows == 0 writes nothing
    assert (out == 1).all()
    pop.close()
