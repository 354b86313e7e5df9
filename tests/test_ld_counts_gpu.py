"""kgx_ld_counts on the device against the plain product: codes [n][G] -> Z = [codes == 1, codes == 2, codes == 3] as int64, the
full Z Z^T over the genomes between the listed rows, read at (i, i + d), zeros past the list's end.  Every word of every entry.

400 rows; G in {37, 65, 600, 2100}: one partial chunk; a one-genome tail chunk; ten chunks = two segments, the second guarded, on
a pitch of 160 that is not line-aligned; a 640-byte line-aligned pitch and five segments.  (n_rows, window): below, at and past one
64-row block, a band ending inside the diagonal block, the next and the one after, a window past the list."""
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 400
SHAPES = [(1, 0), (1, 5), (64, 63), (65, 1), (65, 64), (200, 65), (200, 130), (200, 300)]


@lru_cache(maxsize=None)
def codes_of(G):
    rng = np.random.default_rng(9000 + G)
    codes = rng.choice(4, size=(V, G), p=[0.6, 0.2, 0.15, 0.05]).astype(np.uint8)
    codes[1], codes[2], codes[3] = 2, 3, 0                     # all minor homozygous, never called, all reference
    codes[4:8, G - 1] = [0, 1, 2, 3]                           # the last genome of the last chunk carries every kind
    return codes


@lru_cache(maxsize=None)
def row_list(n_rows):
    rows = np.random.default_rng(n_rows).permutation(V)[:n_rows].astype(np.uint32)   # shuffled, not adjacent
    if n_rows > 1:
        rows[-1] = rows[0]                                     # ... and one row twice
    return rows


def band(codes, window):
    n = len(codes)                                             # -> [n][window + 1][9] uint32 over the genomes of codes [n][G]
    Z = np.stack([codes == 1, codes == 2, codes == 3]).astype(np.int64)          # [kind][row][genome]
    full = np.einsum("pig,qjg->ijpq", Z, Z).reshape(n, n, 9)
    table = np.zeros((n, window + 1, 9), dtype=np.uint32)
    for d in range(min(window + 1, n)):
        table[np.arange(n - d), d] = full[np.arange(n - d), np.arange(d, n)]
    return table


@lru_cache(maxsize=None)
def expected(G, n_rows, window, listed):
    return band(codes_of(G)[row_list(n_rows)] if listed else codes_of(G)[:n_rows], window)


def population(kgx, codes):
    pop = kgx.Population(codes.shape[1], codes.shape[0])
    pop.load_dosage2(kgx.pack_dosage2(codes))
    return pop


def assert_same(got, want):
    assert got.shape == want.shape and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("n_rows,window", SHAPES)
@pytest.mark.parametrize("G", [37, 65, 600, 2100])
def test_every_word_equals_the_product(kgx, G, n_rows, window, listed):
    pop = population(kgx, codes_of(G))
    got = pop.ld_counts(row_list(n_rows) if listed else None, n_rows, window)
    pop.close()
    assert_same(got, expected(G, n_rows, window, listed))


def test_genome_mask(kgx):
    G, window = 600, 65
    codes = codes_of(G)
    keep = (np.arange(G) % 7 != 0).astype(np.uint8)
    pop = population(kgx, codes)
    pop.set_genome_mask(keep)
    got = pop.ld_counts(window=window)
    by_locus = pop.allele_count_by_locus()
    pop.close()
    assert_same(got, band(codes * keep, window))
    assert np.array_equal(got[:, 0][:, [0, 4, 8]], by_locus[:, 1:4])


@pytest.fixture
def rebind(kgx):
    yield kgx.init
    kgx.init(0)


def test_one_device_listed_three_times(kgx, rebind):
    G = 600
    rebind([0, 0, 0])
    pop = population(kgx, codes_of(G))
    assert len([s for s in pop.shards if s["n_genomes"]]) == 3
    got = pop.ld_counts(row_list(200), window=130)
    pop.close()
    assert_same(got, expected(G, 200, 130, True))


@pytest.mark.parametrize("switch,value,batches,splits", [("KGX_LD_ROWS", "64", 4, 5), ("KGX_LD_ROWS", "7", 4, 5), ("KGX_LD_SPLITS", "1", 1, 1),
                                                        ("KGX_LD_SPLITS", "2", 1, 2)])
def test_batches_and_slices_change_nothing(kgx, monkeypatch, switch, value, batches, splits):
    """G = 2100 is five segments; 200 rows are four blocks, 16 block pairs at most: without a cap a slice per segment.  A cap of 7
    rows is one block a batch (store, then the next batch's table); KGX_LD_SPLITS=1 walks the five segments in one workgroup and
    stores plainly, =2 as three and two."""
    G = 2100
    pop = population(kgx, codes_of(G))
    monkeypatch.setenv(switch, value)
    kgx.reload_options()
    try:
        got = pop.ld_counts(row_list(200), window=130)
        ms, reported_batches, reported_splits = kgx.ld_counts_last()
    finally:
        monkeypatch.delenv(switch)
        kgx.reload_options()
        pop.close()
    assert (reported_batches, reported_splits) == (batches, splits) and ms > 0.0
    assert_same(got, expected(G, 200, 130, True))


def test_one_block_pair_splits_its_genomes(kgx):
    G = 2100
    pop = population(kgx, codes_of(G))
    got = pop.ld_counts(n_rows=64, window=63)
    _, batches, splits = kgx.ld_counts_last()
    pop.close()
    assert batches == 1 and splits == 5                        # one block pair: a slice per 512-genome segment
    assert_same(got, expected(G, 64, 63, False))


def test_refusals(kgx):
    G = 37
    pop = population(kgx, codes_of(G))
    out = np.ones((V, 3, 9), dtype=np.uint32)
    rows = np.array([5, V], dtype=np.uint32)
    assert kgx.lib().kgx_ld_counts(pop._h, kgx.ptr(rows), 2, 2, kgx.ptr(out)) == kgx.KGX_EINVAL
    assert "rows[1]" in kgx.lib().kgx_last_error().decode()
    assert kgx.lib().kgx_ld_counts(pop._h, None, V + 1, 2, kgx.ptr(out)) == kgx.KGX_EINVAL
    assert kgx.lib().kgx_ld_counts(pop._h, None, V, 2, None) == kgx.KGX_EINVAL
    assert kgx.lib().kgx_ld_counts(pop._h, None, 0, 2, kgx.ptr(out)) == kgx.KGX_OK and out.all()   # n_rows == 0 writes nothing
    pop.close()
