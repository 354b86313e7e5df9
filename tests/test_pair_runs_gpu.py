"""kgx_pair_runs on the device against the walk of include/kgx.h, written as a plain loop over the rows and vectorised over the
pairs: every summary word of every pair, as integers.

1100 rows (three staged chunks of 512); random codes plus crafted genomes: all 0; a copy of it with code 2 on both sides of every
64-tile edge; all 3; all 0 with no-calls at the ends of runs, of the list and across the first chunk's end (its open run against
genome 0 is closed by the break at 520, a chunk after its last site); all 1 (never a mismatch under IBS0, always one under IDENTICAL
against homozygotes); all 2 with two 0s.  G in {20, 33, 130}: one partial 32-genome tile; a one-genome tail tile; five tiles, so
diagonal and off-diagonal tile pairs and three 64-genome panel chunks.  The shapes are those of test_roh_gpu.py (1, 64, 65 and 400
rows, min_sites 63 and 64, a gap rule) and two of 1100 rows."""
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 1100
SHAPES = [(1, 1, 1, 0), (64, 1, 1, 0), (65, 2, 1, 0), (200, 10, 5000, 20000), (400, 25, 20000, 20000), (400, 1, 1, 0), (400, 63, 1, 0),
          (400, 64, 1, 20000), (1100, 1, 1, 0), (1100, 64, 20000, 20000)]
BIG = (400, 25, 20000, 20000)


@lru_cache(maxsize=None)
def codes_of(G):
    codes = np.random.default_rng(9000 + G).choice(4, size=(V, G), p=[0.70, 0.03, 0.22, 0.05]).astype(np.uint8)
    edges = np.arange(64, V, 64)
    codes[:, 0] = 0
    codes[:, 1] = 0
    codes[np.concatenate([edges - 1, edges]), 1] = 2           # mismatches on both sides of every tile edge
    codes[:, 2] = 3                                            # never called: no run with anybody
    codes[:, 3] = 0
    codes[[0, 1, 62, 63, 64, *range(120, 136), 399, *range(505, 526), V - 1], 3] = 3
    codes[200, 3] = 2
    codes[:, 4] = 1
    codes[:, G - 1] = 2
    codes[[10, 300], G - 1] = 0
    return codes


@lru_cache(maxsize=None)
def positions(n):
    step = np.random.default_rng(n).integers(1, 2000, size=n)
    step[n // 3] = 50_000
    position = np.cumsum(step).astype(np.uint32)
    start = np.zeros(n, dtype=np.uint8)
    for at in (150, 520, 576):                                 # further contigs (576: on a tile edge): positions start again
        if n > at:
            start[at] = 1
            position[at:] -= position[at] - 5
    return position, start


@lru_cache(maxsize=None)
def row_list(n_rows):
    rows = np.random.default_rng(n_rows).permutation(V)[:n_rows].astype(np.uint32)   # shuffled, not adjacent
    if n_rows > 1:
        rows[-1] = rows[0]                                     # ... and one row twice
    return rows


def walk(codes, position, start, min_sites, min_length, max_gap, mode):
    """[G (G + 1) / 2][4]: the walk of include/kgx.h, row by row, all pairs at once."""
    n_rows, G = codes.shape
    position = position.astype(np.int64)
    a, b = np.triu_indices(G)                                  # row-major over a <= b: the pair index
    first, last, sites = (np.zeros(len(a), dtype=np.int64) for _ in range(3))
    open_ = np.zeros(len(a), dtype=bool)
    out = np.zeros((len(a), 4), dtype=np.uint64)

    def close(which):
        which = which & open_
        length = position[last] - position[first] + 1
        kept = which & (sites >= max(min_sites, 1)) & (length >= max(min_length, 1))
        out[kept, 0] += np.uint64(1)
        out[kept, 1] += length[kept].astype(np.uint64)
        out[kept, 2] = np.maximum(out[kept, 2], length[kept].astype(np.uint64))
        out[kept, 3] += sites[kept].astype(np.uint64)
        open_[which] = False

    for i in range(n_rows):
        if i and (start[i] or (max_gap and position[i] - position[i - 1] > max_gap)):
            close(~np.zeros(len(a), dtype=bool))
        ca, cb = codes[i, a].astype(np.int64), codes[i, b].astype(np.int64)
        nocall = (ca == 3) | (cb == 3)
        mismatch = ~nocall & ((ca != cb) if mode else (np.minimum(ca, cb) == 0) & (np.maximum(ca, cb) == 2))
        close(mismatch)
        shared = ~nocall & ~mismatch
        opened = shared & ~open_
        first[opened], sites[opened], open_[opened] = i, 0, True
        last[shared] = i
        sites[shared] += 1
    close(~np.zeros(len(a), dtype=bool))
    return out


@lru_cache(maxsize=None)
def expected(G, n_rows, min_sites, min_length, max_gap, mode, listed):
    codes = codes_of(G)[row_list(n_rows)] if listed else codes_of(G)[:n_rows]
    want = walk(codes, *positions(n_rows), min_sites, min_length, max_gap, mode)
    want.setflags(write=False)
    return want


def population(kgx, codes):
    pop = kgx.Population(codes.shape[1], codes.shape[0])
    pop.load_dosage2(kgx.pack_dosage2(codes))
    return pop


def pair_runs(pop, n_rows, min_sites, min_length, max_gap, mode, listed):
    position, start = positions(n_rows)
    return pop.pair_runs(position, row_list(n_rows) if listed else None, n_rows, start, min_sites, min_length, max_gap, mode)


def assert_same(got, want, n_rows=400, min_sites=1):
    assert (want[:, 0] > 0).any() or (n_rows == 1 and min_sites > 1)
    assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:10]


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n_rows,min_sites,min_length,max_gap", SHAPES)
@pytest.mark.parametrize("G", [20, 33, 130])
def test_every_summary_equals_the_walk(kgx, G, n_rows, min_sites, min_length, max_gap, mode, listed):
    pop = population(kgx, codes_of(G))
    got = pair_runs(pop, n_rows, min_sites, min_length, max_gap, mode, listed)
    pop.close()
    assert_same(got, expected(G, n_rows, min_sites, min_length, max_gap, mode, listed), n_rows, min_sites)


def test_the_two_modes_differ():
    """From the reference alone: a het against a homozygote is shared under IBS0 and a mismatch under IDENTICAL."""
    ibs0, identical = expected(33, *BIG, 0, False), expected(33, *BIG, 1, False)
    assert not np.array_equal(ibs0, identical)
    het_hom = 0 * 33 + 4                                       # pair (0, 4): all 0 against all 1
    assert ibs0[het_hom, 0] > 0 and identical[het_hom, 0] == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("min_sites", [63, 64])
def test_breaks_on_tile_edges(kgx, mode, min_sites):
    """Contig starts at 64 and 128, and genome 1 against genome 0 mismatching at 63, 127, 191 and 255: the pair's runs {64, 126} and
    {128, 190} lie between a break at bit 0 and a mismatch at bit 63 of one tile -- 63 sites, the most a run inside a tile can have."""
    G, n = 33, 256
    codes = codes_of(G)[:n].copy()
    codes[[64, 128, 192], 1] = 0
    position = np.arange(1, n + 1, dtype=np.uint32) * 100
    start = np.zeros(n, dtype=np.uint8)
    start[[64, 128]] = 1
    want = walk(codes, position, start, min_sites, 1, 0, mode)
    assert want[1].tolist() == ([4, 4 * 6201, 6201, 4 * 63] if min_sites == 63 else [0, 0, 0, 0])      # pair (0, 1)
    pop = population(kgx, codes)
    got = pop.pair_runs(position, None, n, start, min_sites, 1, 0, mode)
    pop.close()
    assert_same(got, want)


def test_genome_mask(kgx):
    G = 130
    keep = (np.arange(G) % 7 != 0).astype(np.uint8)
    pop = population(kgx, codes_of(G))
    pop.set_genome_mask(keep)
    got = pair_runs(pop, *BIG, 1, False)
    pop.close()
    a, b = np.triu_indices(G)
    want = expected(G, *BIG, 1, False) * (keep[a] & keep[b]).astype(np.uint64)[:, None]
    assert_same(got, want)


@pytest.fixture
def rebind(kgx):
    yield kgx.init
    kgx.init(0)


def test_one_device_listed_three_times(kgx, rebind):
    G = 130
    rebind([0, 0, 0])
    pop = population(kgx, codes_of(G))
    assert len([s for s in pop.shards if s["n_genomes"]]) == 3
    got = pair_runs(pop, *BIG, 0, True)
    pop.close()
    assert_same(got, expected(G, *BIG, 0, True))


@pytest.mark.parametrize("cap,batches", [("64", 7), ("128", 4), ("100", 4), (None, 1)])
def test_batches_change_nothing(kgx, monkeypatch, cap, batches):
    """KGX_PAIR_RUNS_ROWS=64: a batch a tile -- every run that crosses a tile edge is carried by the table, and the run of (0, 3) that
    the break at 133 closes had its last site, 119, a batch earlier; 100 is rounded up to 128."""
    G = 130
    pop = population(kgx, codes_of(G))
    if cap:
        monkeypatch.setenv("KGX_PAIR_RUNS_ROWS", cap)
    kgx.reload_options()
    try:
        got = pair_runs(pop, *BIG, 0, False)
        ms, reported = kgx.pair_runs_last()
    finally:
        monkeypatch.delenv("KGX_PAIR_RUNS_ROWS", raising=False)
        kgx.reload_options()
        pop.close()
    assert reported == batches and ms > 0.0
    assert_same(got, expected(G, *BIG, 0, False))


def test_refusals(kgx):
    G = 33
    pop = population(kgx, codes_of(G))
    position, start = positions(V)
    out = np.ones((G * (G + 1) // 2, 4), dtype=np.uint64)

    def call(rows, n_rows, pos, starts, o=out, mode=0, handle=pop._h):
        params = np.array([1, 1, 0, mode], dtype=np.uint32)
        return kgx.lib().kgx_pair_runs(handle, None if rows is None else kgx.ptr(rows), n_rows, None if pos is None else kgx.ptr(pos),
                                       None if starts is None else kgx.ptr(starts), kgx.ptr(params), None if o is None else kgx.ptr(o))

    assert call(np.array([5, V], dtype=np.uint32), 2, position, start) == kgx.KGX_EINVAL
    assert "rows[1]" in kgx.lib().kgx_last_error().decode()
    assert call(None, V + 1, position, start) == kgx.KGX_EINVAL
    assert call(None, 1 << 32, position, start) == kgx.KGX_EINVAL
    assert call(None, V, position, None) == kgx.KGX_EINVAL       # positions start again at 150: not without its contig start
    assert "position[150]" in kgx.lib().kgx_last_error().decode()
    assert call(None, V, None, start) == kgx.KGX_EINVAL and call(None, V, position, start, o=None) == kgx.KGX_EINVAL
    assert call(None, V, position, start, handle=None) == kgx.KGX_EINVAL
    assert call(None, V, position, start, mode=2) == kgx.KGX_EINVAL and "mode 2" in kgx.lib().kgx_last_error().decode()
    assert call(None, V, position, start) == kgx.KGX_OK and out[:, 0].any()
    assert call(None, 0, None, None) == kgx.KGX_OK and not out.any()                                  # n_rows == 0: zeros
    pop.close()
