"""kgx_roh on the device against the walk of include/kgx.h written as a plain loop per genome: every summary field, begin and every
segment triple, as integers.

400 rows; G in {37, 65, 300, 2100}: one partial chunk; a one-genome tail chunk; a second, partial column wave; a line-aligned pitch.
Five crafted genomes put hets on both sides of every tile edge and no-calls at the ends of runs and of the list.  (n_rows, min_sites,
min_length, max_gap): below, at and past one 64-position tile, lists of several tiles with and without a filter and a gap rule, and
min_sites 63 and 64: the last value at which the kernel looks at the runs between two events of one tile, and the first at which
it passes over them.  A second list puts contig starts on tile edges, where such a run is longest: 63 sites."""
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 400
SHAPES = [(1, 1, 1, 0), (64, 1, 1, 0), (65, 2, 1, 0), (200, 10, 5000, 20000), (400, 25, 20000, 20000), (400, 1, 1, 0), (400, 63, 1, 0),
          (400, 64, 1, 20000)]


@lru_cache(maxsize=None)
def codes_of(G):
    codes = np.random.default_rng(7000 + G).choice(4, size=(V, G), p=[0.70, 0.03, 0.22, 0.05]).astype(np.uint8)
    codes[:, 0] = 0                                            # one run through everything the breaks allow
    codes[:, 1] = 3                                            # never called: no run
    codes[:, 2] = 0
    codes[[63, 64, 65, 127, 128, 191, 192], 2] = 1             # hets on both sides of every tile edge
    codes[:, 3] = 0
    codes[[0, 1, 62, 63, 64, 130, 131, 399], 3] = 3            # no-calls at the ends of runs and of the list
    codes[200, 3] = 1
    codes[:, G - 1] = 2
    codes[[10, 300], G - 1] = 1
    return codes


@lru_cache(maxsize=None)
def positions(n):
    step = np.random.default_rng(n).integers(1, 2000, size=n)
    step[n // 3] = 50_000
    position = np.cumsum(step).astype(np.uint32)
    start = np.zeros(n, dtype=np.uint8)
    if n > 150:
        start[150] = 1                                         # a second contig: positions start again
        position[150:] -= position[150] - 5
    return position, start


@lru_cache(maxsize=None)
def row_list(n_rows):
    rows = np.random.default_rng(n_rows).permutation(V)[:n_rows].astype(np.uint32)   # shuffled, not adjacent
    if n_rows > 1:
        rows[-1] = rows[0]                                     # ... and one row twice
    return rows


def walk(column, position, start, min_sites, min_length, max_gap):
    runs, run = [], None                                       # run = [first, last, sites]

    def close():
        nonlocal run
        if run and run[2] >= min_sites and int(position[run[1]]) - int(position[run[0]]) + 1 >= min_length:
            runs.append(tuple(run))
        run = None

    for i, code in enumerate(column):
        if i and (start[i] or (max_gap and int(position[i]) - int(position[i - 1]) > max_gap)):
            close()
        if code == 1:
            close()
        elif code != 3:
            run = [run[0], i, run[2] + 1] if run else [i, i, 1]
    close()
    return runs


def tables(runs_of, position):
    """(summary [G][4], begin [G + 1], segments [..][3]) of per-genome run lists."""
    summary = np.zeros((len(runs_of), 4), dtype=np.uint64)
    for g, runs in enumerate(runs_of):
        lengths = [int(position[last]) - int(position[first]) + 1 for first, last, _ in runs]
        summary[g] = [len(runs), sum(lengths), max(lengths, default=0), sum(sites for _, _, sites in runs)]
    begin = np.concatenate([[0], np.cumsum(summary[:, 0])]).astype(np.uint64)
    segments = np.array([r for runs in runs_of for r in runs], dtype=np.uint32).reshape(-1, 3)
    return summary, begin, segments


@lru_cache(maxsize=None)
def runs_of(G, n_rows, min_sites, min_length, max_gap, listed):
    codes = codes_of(G)[row_list(n_rows)] if listed else codes_of(G)[:n_rows]
    position, start = positions(n_rows)
    return [walk(codes[:, g].tolist(), position, start, min_sites, min_length, max_gap) for g in range(G)]


def expected(G, n_rows, min_sites, min_length, max_gap, listed):
    return tables(runs_of(G, n_rows, min_sites, min_length, max_gap, listed), positions(n_rows)[0])


def population(kgx, codes):
    pop = kgx.Population(codes.shape[1], codes.shape[0])
    pop.load_dosage2(kgx.pack_dosage2(codes))
    return pop


def roh(pop, n_rows, min_sites, min_length, max_gap, listed, **more):
    position, start = positions(n_rows)
    return pop.roh(position, row_list(n_rows) if listed else None, n_rows, start, min_sites, min_length, max_gap, **more)


def assert_same(got, want):
    summary, begin, segments = got
    fields = np.stack([summary[name] for name in ("runs", "total_length", "longest_length", "sites_in_runs")], axis=1)
    assert np.array_equal(fields, want[0]), np.argwhere(fields != want[0])[:10]
    assert begin.dtype == np.uint64 and np.array_equal(begin, want[1]), np.argwhere(begin != want[1])[:10]
    assert segments.dtype == np.uint32 and segments.shape == want[2].shape and np.array_equal(segments, want[2]), np.argwhere(segments != want[2])[:10]


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("n_rows,min_sites,min_length,max_gap", SHAPES)
@pytest.mark.parametrize("G", [37, 65, 300, 2100])
def test_every_run_equals_the_walk(kgx, G, n_rows, min_sites, min_length, max_gap, listed):
    pop = population(kgx, codes_of(G))
    got = roh(pop, n_rows, min_sites, min_length, max_gap, listed)
    pop.close()
    assert_same(got, expected(G, n_rows, min_sites, min_length, max_gap, listed))


def test_the_inputs_hold_every_class_of_run():
    """From the reference alone: the filter keeps some runs and drops others, runs cross tile edges and lie over three tiles or more."""
    kept = [r for runs in runs_of(37, 400, 25, 20000, 20000, False) for r in runs]
    unfiltered = [r for runs in runs_of(37, 400, 1, 1, 20000, False) for r in runs]
    assert 0 < len(kept) < len(unfiltered)
    assert any(first // 64 != last // 64 for first, last, _ in kept)
    assert any(last // 64 - first // 64 >= 2 for first, last, _ in kept)
    assert max(last - first + 1 for first, last, _ in unfiltered) >= 250


@pytest.mark.parametrize("min_sites", [63, 64])
def test_breaks_on_tile_edges(kgx, min_sites):
    """Contig starts at 64 and 128, and genome 0 all code 0 with hets at 127 and 191: its runs {64, 126} and {128, 190} lie between a
    break at bit 0 and a het at bit 63 of one tile -- 63 sites, the most a run inside a tile can have."""
    G, n = 65, 256
    codes = codes_of(G)[:n].copy()
    codes[:, 0] = 0
    codes[[127, 191], 0] = 1
    position = np.arange(1, n + 1, dtype=np.uint32) * 100
    start = np.zeros(n, dtype=np.uint8)
    start[[64, 128]] = 1
    want = [walk(codes[:, g].tolist(), position, start, min_sites, 1, 0) for g in range(G)]
    assert [sites for _, _, sites in want[0]] == ([64, 63, 63, 64] if min_sites == 63 else [64, 64])
    pop = population(kgx, codes)
    got = pop.roh(position, None, n, start, min_sites, 1, 0)
    pop.close()
    assert_same(got, tables(want, position))


@pytest.mark.parametrize("cap,slices", [("1", 1), ("2", 2), (None, 7)])
def test_slices_change_nothing(kgx, monkeypatch, cap, slices):
    """400 positions are seven tiles: a slice each without a cap (ten column waves leave the device idle otherwise); KGX_ROH_SLICES=2
    walks four and three tiles a slice and stitches once, =1 carries every run through the registers alone."""
    G = 2100
    pop = population(kgx, codes_of(G))
    if cap:
        monkeypatch.setenv("KGX_ROH_SLICES", cap)
    kgx.reload_options()
    try:
        got = roh(pop, 400, 25, 20000, 20000, True)
        ms, reported = kgx.roh_last()
    finally:
        monkeypatch.delenv("KGX_ROH_SLICES", raising=False)
        kgx.reload_options()
        pop.close()
    assert reported == slices and ms > 0.0
    assert_same(got, expected(G, 400, 25, 20000, 20000, True))


def test_genome_mask(kgx):
    G = 300
    keep = (np.arange(G) % 7 != 0).astype(np.uint8)
    pop = population(kgx, codes_of(G))
    pop.set_genome_mask(keep)
    got = roh(pop, 400, 1, 1, 0, False)
    pop.close()
    assert_same(got, tables([runs if keep[g] else [] for g, runs in enumerate(runs_of(G, 400, 1, 1, 0, False))], positions(400)[0]))


@pytest.fixture
def rebind(kgx):
    yield kgx.init
    kgx.init(0)


def test_one_device_listed_three_times(kgx, rebind):
    G = 300
    rebind([0, 0, 0])
    pop = population(kgx, codes_of(G))
    assert len([s for s in pop.shards if s["n_genomes"]]) == 3
    got = roh(pop, 400, 25, 20000, 20000, True)
    pop.close()
    assert_same(got, expected(G, 400, 25, 20000, 20000, True))


def test_summaries_alone(kgx):
    G = 300
    pop = population(kgx, codes_of(G))
    summary, begin, segments = roh(pop, 400, 25, 20000, 20000, False, runs=False)
    full = roh(pop, 400, 25, 20000, 20000, False)
    pop.close()
    assert begin is None and segments is None and np.array_equal(summary, full[0]) and summary["runs"].sum() > 0


def test_refusals(kgx):
    G = 300
    pop = population(kgx, codes_of(G))
    position, start = positions(V)
    summary, begin = np.ones(G, dtype=kgx.ROH_SUMMARY), np.ones(G + 1, dtype=np.uint64)
    params = np.array([1, 1, 0], dtype=np.uint32)

    def call(rows, n_rows, pos, starts, s=summary, b=begin, segments=None, capacity=0, handle=pop._h):
        return kgx.lib().kgx_roh(handle, None if rows is None else kgx.ptr(rows), n_rows, None if pos is None else kgx.ptr(pos),
                                 None if starts is None else kgx.ptr(starts), kgx.ptr(params), None if s is None else kgx.ptr(s),
                                 None if b is None else kgx.ptr(b), None if segments is None else kgx.ptr(segments), capacity)

    assert call(np.array([5, V], dtype=np.uint32), 2, position, start) == kgx.KGX_EINVAL
    assert "rows[1]" in kgx.lib().kgx_last_error().decode()
    assert call(None, V + 1, position, start) == kgx.KGX_EINVAL
    assert call(None, 1 << 32, position, start) == kgx.KGX_EINVAL
    assert call(None, V, position, None) == kgx.KGX_EINVAL       # positions start again at 150: not without its contig start
    assert "position[150]" in kgx.lib().kgx_last_error().decode()
    assert call(None, V, None, start) == kgx.KGX_EINVAL and call(None, V, position, start, s=None) == kgx.KGX_EINVAL
    assert call(None, V, position, start, handle=None) == kgx.KGX_EINVAL
    assert call(None, V, position, start) == kgx.KGX_OK and begin[G] > 0
    short = np.zeros((int(begin[G]) - 1, 3), dtype=np.uint32)
    assert call(None, V, position, start, segments=short, capacity=len(short)) == kgx.KGX_EINVAL
    assert call(None, 0, None, None) == kgx.KGX_OK and not begin.any() and not summary["runs"].any()   # n_rows == 0: zeros
    pop.close()
