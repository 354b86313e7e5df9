"""kgx_genome_scores on the device against the plain product: codes [n][G] -> Z = [codes == 1, codes == 2, codes == 3] as int64,
einsum with the int64 weights by list position.  Every word, no tolerance: the result is an integer.

800 rows with the code distribution and special rows of test_column_sums_gpu.py; G in {37, 65, 600, 2100}: one partial chunk; a
second wave with one genome; pitch 160 = 10 chunks = 2 1/2 workgroups, the last workgroup's upper waves are past the pitch; 33
chunks, 9 workgroups.  n_rows below, at and past a 64-row step and a 256-row segment, and several segments (which the grid splits
into slices that add atomically).  n_columns 1, 16, 17, 40: a partial group, one group, a group and one column, three groups."""
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 800
MAX = 8128
EDGES = [0, 63, 64, 65, 127, 128, 8127, 8128]


@lru_cache(maxsize=None)
def codes_of(G):
    rng = np.random.default_rng(9000 + G)
    codes = rng.choice(4, size=(V, G), p=[0.6, 0.2, 0.15, 0.05]).astype(np.uint8)
    codes[1], codes[2], codes[3] = 2, 3, 0                     # all minor homozygous, never called, all reference
    codes[4:8, G - 1] = [0, 1, 2, 3]                           # the last genome of the last chunk carries every kind
    return codes


@lru_cache(maxsize=None)
def weights_of(n_rows, C, mixed=False):
    rng = np.random.default_rng(77 * n_rows + C)
    w = rng.integers(-MAX, MAX + 1, size=(C, n_rows)).astype(np.int16)
    planted = np.array([s * e for e in EDGES for s in (1, -1)], dtype=np.int16)
    at = rng.permutation(C * (n_rows - 1))[:len(planted)]      # the digit edges, anywhere but the last list position
    w[at // max(n_rows - 1, 1), at % max(n_rows - 1, 1)] = planted[:len(at)]
    w[:, n_rows - 1] = np.where(np.arange(C) % 2, -MAX, MAX)
    if mixed:                                                  # a group of one digit between two of two
        w[16:32] = rng.integers(-64, 64, size=(16, n_rows))
        w[16, :2] = [-64, 63]
    return w


@lru_cache(maxsize=None)
def row_list(n_rows):
    rows = np.random.default_rng(n_rows).permutation(V)[:n_rows].astype(np.uint32)   # shuffled, not adjacent
    if n_rows > 1:
        rows[-1] = rows[0]                                     # ... and one row twice
    return rows


def product(codes, weights):
    Z = np.stack([codes == 1, codes == 2, codes == 3]).astype(np.int64)
    return np.einsum("kig,ji->gjk", Z, weights.astype(np.int64), optimize=True)


def population(kgx, codes):
    pop = kgx.Population(codes.shape[1], codes.shape[0])
    pop.load_dosage2(kgx.pack_dosage2(codes))
    return pop


def assert_same(got, want):
    assert got.shape == want.shape and got.dtype == np.int64
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("C", [1, 16, 17, 40])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 256, 257, 700])
@pytest.mark.parametrize("G", [37, 65, 600, 2100])
def test_every_word_equals_the_product(kgx, G, n_rows, C, listed):
    pop = population(kgx, codes_of(G))
    got = pop.genome_scores(weights_of(n_rows, C), row_list(n_rows) if listed else None)
    pop.close()
    assert_same(got, product(codes_of(G)[row_list(n_rows) if listed else slice(n_rows)], weights_of(n_rows, C)))


def test_a_one_digit_group_beside_two_digit_groups(kgx):
    G, C, n_rows = 600, 40, 700
    weights = weights_of(n_rows, C, True)
    assert np.abs(weights[16:32]).max() == 64 and weights[16:32].max() == 63 and np.abs(weights[:16]).max() > 64 and np.abs(weights[32:]).max() > 64
    pop = population(kgx, codes_of(G))
    got = pop.genome_scores(weights, row_list(n_rows))
    pop.close()
    assert_same(got, product(codes_of(G)[row_list(n_rows)], weights))


def test_genome_mask(kgx):
    G, C = 600, 17
    keep = (np.arange(G) % 7 != 0).astype(np.uint8)
    weights = weights_of(V, C).copy()
    weights[3] = 1
    pop = population(kgx, codes_of(G))
    pop.set_genome_mask(keep)
    got = pop.genome_scores(weights)
    pop.close()
    assert not got[keep == 0].any()
    assert_same(got, product(codes_of(G), weights) * keep[:, None, None])
    assert np.array_equal(got[keep != 0, 3], np.stack([(codes_of(G) == k).sum(axis=0) for k in (1, 2, 3)], axis=1)[keep != 0])


@pytest.fixture
def rebind(kgx):
    yield kgx.init
    kgx.init(0)


def test_one_device_listed_three_times(kgx, rebind):
    G, C, n_rows = 600, 40, 700
    rebind([0, 0, 0])
    pop = population(kgx, codes_of(G))
    assert len([s for s in pop.shards if s["n_genomes"]]) == 3
    got = pop.genome_scores(weights_of(n_rows, C), row_list(n_rows))
    pop.close()
    assert_same(got, product(codes_of(G)[row_list(n_rows)], weights_of(n_rows, C)))


@pytest.mark.parametrize("switch,value,batches,splits", [("KGX_GSCORE_ROWS", "256", 3, 1), ("KGX_GSCORE_ROWS", "7", 3, 1), ("KGX_GSCORE_SPLITS", "1", 1, 1),
                                                        ("KGX_GSCORE_SPLITS", "2", 1, 2)])
def test_batches_and_slices_change_nothing(kgx, monkeypatch, switch, value, batches, splits):
    """700 list positions are three 256-row segments; G = 2100 is nine 256-genome blocks and 17 columns two groups, 18 workgroups:
    without a cap a slice per segment.  A cap of 256 or of 7 rows is one segment a batch (and nothing left to split);
    KGX_GSCORE_SPLITS=1 walks the three segments in one workgroup and adds plainly, =2 as two and one, atomically."""
    G, C, n_rows = 2100, 17, 700
    pop = population(kgx, codes_of(G))
    monkeypatch.setenv(switch, value)
    kgx.reload_options()
    try:
        got = pop.genome_scores(weights_of(n_rows, C), row_list(n_rows))
        ms, reported_batches, reported_splits = kgx.genome_scores_last()
    finally:
        monkeypatch.delenv(switch)
        kgx.reload_options()
        pop.close()
    assert (reported_batches, reported_splits) == (batches, splits) and ms > 0.0
    assert_same(got, product(codes_of(G)[row_list(n_rows)], weights_of(n_rows, C)))


@pytest.mark.parametrize("case,needle", [("value", "weights[2][5]"), ("negative", "weights[0][7]"), ("row", "rows[1]"), ("n_rows", "n_rows"),
                                         ("no columns", "no columns"), ("2^32", "2^32"), ("pop", "null"), ("out", "null"), ("weights", "null"),
                                         ("overflow", "overflow")])
def test_refusals(kgx, case, needle):
    G, n = 37, 8
    pop = population(kgx, codes_of(G))
    weights = np.zeros((3, V + 1) if case == "n_rows" else (3, n), dtype=np.int16)
    out = np.ones((G, 3, 3), dtype=np.int64)
    rows = np.arange(n, dtype=np.uint32)
    if case == "row":
        rows[1] = V
    if case == "value":
        weights[2, 5] = MAX + 1
    if case == "negative":
        weights[0, 7] = -MAX - 1
    p, r, w, o = pop._h, kgx.ptr(rows), kgx.ptr(weights), kgx.ptr(out)
    args = {"n_rows": (p, None, V + 1, w, 3, o), "no columns": (p, r, n, w, 0, o), "2^32": (p, r, 1 << 32, w, 3, o), "pop": (None, r, n, w, 3, o),
            "out": (p, r, n, w, 3, None), "weights": (p, r, n, None, 3, o), "overflow": (p, r, (1 << 32) - 1, w, (1 << 32) - 1, o)}
    assert kgx.lib().kgx_genome_scores(*args.get(case, (p, r, n, w, 3, o))) == kgx.KGX_EINVAL
    assert needle in kgx.lib().kgx_last_error().decode()
    assert kgx.lib().kgx_genome_scores(p, None, 0, w, 3, o) == kgx.KGX_OK                                   # n_rows == 0 writes zeros
    assert (out == 0).all()
    pop.close()
