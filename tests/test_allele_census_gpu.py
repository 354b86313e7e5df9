"""kgx_gt8_allele_census on the device against the NumPy restatement (tests/allele_census_reference.py), every word.

Populations are built cell by cell (L = 600 loci, G in {37, 257, 1000}: a tail inside one 16-byte chunk, more than one 128-genome
unit, several shards), mostly 0x00 with whole all-zero stretches, and carry the cells the semantics hinge on: see `build_case`.
"""
from functools import lru_cache

import numpy as np
import pytest

from tests import allele_census_reference as acr

pytestmark = pytest.mark.gpu

L = 600
SHAPES = [(1, 1), (6, 3), (32, 14), (5, 7)]                   # (n_groups, amax): 5, 9, 31 and 17 kinds -- none divides a tile of 16 rows


def cell(lo, hi):
    return np.uint8(lo | (hi << 4))


@lru_cache(maxsize=None)
def build_case(G):
    """cells [L][G] uint8 and the rows the special cells sit in."""
    rng = np.random.default_rng(4000 + G)
    lo = rng.choice(16, size=(L, G), p=[0.55, 0.15, 0.08, 0.05] + [0.01] * 11 + [0.06]).astype(np.uint8)
    hi = rng.choice(16, size=(L, G), p=[0.70, 0.10, 0.06, 0.03] + [0.005] * 11 + [0.055]).astype(np.uint8)
    cells = (lo | (hi << 4)).astype(np.uint8)
    cells[rng.random((L, G)) < 0.6] = 0                        # mostly reference
    cells[100:180] = 0                                         # a stretch nobody carries anything in
    cells[:, G // 2:G // 2 + 8][300:420] = 0                   # ... and chunks that are empty for many loci
    cells[:20] = 0
    a, b = 2, 3
    planted = [cell(a, 0), cell(a, a), cell(0, a), cell(a, b), cell(b, a), cell(15, 0), cell(a, 15), cell(15, a), cell(15, 15), cell(0, 15),
               np.uint8(0xFF), cell(5, 0), cell(0, 5), cell(5, 5), cell(5, 1), cell(14, 14), cell(0, 14)]
    for i, byte in enumerate(planted):                         # locus 1: in the first genomes; locus 2: in the last (the tail of a chunk)
        cells[1, i % G] = byte
        cells[2, G - 1 - (i % G)] = byte
    cells[3] = 0xFF                                            # crowded throughout
    cells[4] = cell(1, 1)                                      # everybody holds (a, a): counts past 255 and 2 G / 2 at G = 1000
    cells[5] = cell(0, 1)
    cells[L - 1] = cell(3, 3)                                  # the last locus: the partial last tile
    cells.setflags(write=False)
    return cells


def groups_of(G, n_groups):
    """Group n_groups - 2 (where there is one) has no genome; every 11th genome is in no group; at n_groups == 1 all the others are in group 0."""
    rng = np.random.default_rng(n_groups)
    usable = [g for g in range(n_groups) if n_groups < 3 or g != n_groups - 2]
    groups = rng.choice(usable, G).astype(np.uint8)
    groups[::11] = 0xFF
    return groups


def one_group_holds_all(G, n_groups):
    groups = np.full(G, n_groups - 1, dtype=np.uint8)
    return groups


@lru_cache(maxsize=None)
def expected(G, n_groups, amax):
    want = acr.census(build_case(G), groups_of(G, n_groups), n_groups, amax)
    want.setflags(write=False)
    return want


def matrix(kgx, cells):
    m = kgx.GenotypeMatrix(cells.shape[1], cells.shape[0])
    m.load_rows(cells)
    return m


SUBSET = np.sort(np.random.default_rng(9).choice(L, 257, replace=False)).astype(np.uint32)


@pytest.mark.parametrize("G", [37, 257, 1000])
@pytest.mark.parametrize("n_groups,amax", SHAPES)
def test_census_equals_the_numpy_restatement(kgx, G, n_groups, amax):
    cells = build_case(G)
    groups = groups_of(G, n_groups)
    want = expected(G, n_groups, amax)
    m = matrix(kgx, cells)
    got = m.allele_census(groups, n_groups, amax)
    assert got.shape == want.shape == (L, n_groups, 3 + 2 * amax)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10]
    ms, batches = kgx.allele_census_last()
    assert batches == 1 and ms > 0.0
    sub = m.allele_census(groups, n_groups, amax, locus_index=SUBSET)
    assert np.array_equal(sub, want[SUBSET]), np.argwhere(sub != want[SUBSET])[:10]
    first = m.allele_census(groups, n_groups, amax, n_selected=301)          # NULL locus_index: rows 0 .. n_selected - 1
    assert np.array_equal(first, want[:301])
    # what the planted loci are there for
    sizes = acr.group_sizes(groups, n_groups)
    assert np.array_equal(got[3, :, 2], sizes) and not got[3][:, [0, 1] + list(range(3, 3 + 2 * amax))].any()   # crowded: no copies counted
    assert np.array_equal(got[4, :, 4], sizes) and not got[4, :, 3].any()      # (1, 1): double_1
    assert np.array_equal(got[5, :, 4], sizes)                                 # (0, 1): that alt twice
    if n_groups >= 3:
        assert not got[:, n_groups - 2].any()                                   # the group without a genome
    if amax == 3:
        assert got[1, :, 1].sum() > 0                                           # index 5 read at amax = 3: unknown copies
    m.close()


@pytest.mark.parametrize("G", [257, 1000])
def test_one_group_holding_every_genome(kgx, G):
    """Every genome holds (1, 1) at locus 4 and one group holds them all: a count of G (past 255) in one word."""
    cells = build_case(G)
    groups = one_group_holds_all(G, 6)
    m = matrix(kgx, cells)
    got = m.allele_census(groups, 6, 3)
    m.close()
    assert np.array_equal(got, acr.census(cells, groups, 6, 3))
    assert got[4, 5, 4] == G and not got[:, :5].any()


def test_against_the_two_bit_allele_count_sweep(kgx):
    """An independent yardstick: the K2 kernel over the same biallelic cells, one genome mask per group."""
    G, n_groups = 1000, 3
    rng = np.random.default_rng(31)
    codes = rng.choice(3, size=(L, G), p=[0.8, 0.13, 0.07]).astype(np.uint8)
    cells = np.where(codes == 1, cell(1, 0), np.where(codes == 2, cell(1, 1), np.uint8(0))).astype(np.uint8)
    groups = rng.integers(0, n_groups, G).astype(np.uint8)
    m = matrix(kgx, cells)
    got = m.allele_census(groups, n_groups, 1)
    m.close()
    pop = kgx.Population(G, L)
    pop.load_dosage2(kgx.pack_dosage2(codes))
    for g in range(n_groups):
        pop.set_genome_mask((groups == g).astype(np.uint8))
        k2 = pop.allele_count_by_locus()                        # { ref, het, hom, non-diploid }
        assert np.array_equal(k2[:, :3], got[:, g, [0, 3, 4]]), g
    pop.close()


@pytest.fixture
def rebind(kgx):
    yield kgx.init
    kgx.init(0)


@pytest.mark.parametrize("G", [37, 257, 1000])
def test_one_device_listed_three_times_gives_identical_bytes(kgx, rebind, G):
    cells = build_case(G)
    rebind([0, 0, 0])
    m = matrix(kgx, cells)
    assert len([s for s in m.shards if s["n_genomes"]]) == min(3, (G + 127) // 128)
    for n_groups, amax in [(6, 3), (32, 14)]:
        got = m.allele_census(groups_of(G, n_groups), n_groups, amax)
        assert got.tobytes() == expected(G, n_groups, amax).tobytes()
        sub = m.allele_census(groups_of(G, n_groups), n_groups, amax, locus_index=SUBSET)
        assert sub.tobytes() == expected(G, n_groups, amax)[SUBSET].tobytes()
    m.close()


@pytest.mark.parametrize("per_batch,batches", [("1", 600), ("64", 10), ("599", 2), (None, 1)])
def test_locus_batches_change_nothing(kgx, monkeypatch, per_batch, batches):
    G, n_groups, amax = 257, 6, 3
    m = matrix(kgx, build_case(G))
    if per_batch is not None:
        monkeypatch.setenv("KGX_CENSUS_LOCI", per_batch)
    kgx.reload_options()
    try:
        got = m.allele_census(groups_of(G, n_groups), n_groups, amax)
        reported = kgx.allele_census_last()[1]
        sub = m.allele_census(groups_of(G, n_groups), n_groups, amax, locus_index=SUBSET)
    finally:
        monkeypatch.delenv("KGX_CENSUS_LOCI", raising=False)
        kgx.reload_options()
        m.close()
    assert reported == batches
    assert got.tobytes() == expected(G, n_groups, amax).tobytes()
    assert sub.tobytes() == expected(G, n_groups, amax)[SUBSET].tobytes()


def test_the_same_bits_on_every_run(kgx):
    G = 1000
    m = matrix(kgx, build_case(G))
    runs = [m.allele_census(groups_of(G, 32), 32, 14).tobytes() for _ in range(3)]
    m.close()
    assert runs[0] == runs[1] == runs[2]


def raw_call(kgx, m, groups, n_groups, amax, locus_index, n_selected):
    out = np.zeros((max(int(n_selected), 1), max(min(int(n_groups), 64), 1), 3 + 2 * max(min(int(amax), 32), 1)), dtype=np.uint32)
    idx = None if locus_index is None else np.ascontiguousarray(locus_index, dtype=np.uint32)
    rc = kgx.lib().kgx_gt8_allele_census(m._h, kgx.ptr(groups), n_groups, None if idx is None else kgx.ptr(idx), n_selected, amax, kgx.ptr(out))
    return rc, kgx.lib().kgx_last_error().decode(), out


def test_refusals_name_the_argument(kgx):
    G = 37
    m = matrix(kgx, build_case(G))
    groups = groups_of(G, 6)
    bad = groups.copy()
    bad[G - 1] = 7
    rc, message, _ = raw_call(kgx, m, bad, 6, 3, None, L)
    assert rc == kgx.KGX_EINVAL and "group_of_genome" in message
    rc, message, _ = raw_call(kgx, m, groups, 33, 3, None, L)
    assert rc == kgx.KGX_EINVAL and "n_groups" in message
    for amax in (0, 15):
        rc, message, _ = raw_call(kgx, m, groups, 6, amax, None, L)
        assert rc == kgx.KGX_EINVAL and "amax" in message
    rc, message, _ = raw_call(kgx, m, groups, 6, 3, [5, 4], 2)
    assert rc == kgx.KGX_EINVAL and "locus_index" in message and "ascending" in message
    rc, message, _ = raw_call(kgx, m, groups, 6, 3, [5, L], 2)
    assert rc == kgx.KGX_EINVAL and "locus_index" in message
    rc, message, _ = raw_call(kgx, m, groups, 6, 3, None, L + 1)
    assert rc == kgx.KGX_EINVAL and "n_selected" in message
    assert kgx.lib().kgx_gt8_allele_census(m._h, None, 6, None, L, 3, None) == kgx.KGX_EINVAL
    # n_selected == 0 with an output buffer: fine, nothing written
    rc, _, out = raw_call(kgx, m, groups, 6, 3, None, 0)
    assert rc == kgx.KGX_OK and not out.any()
    # a selected locus with a wide row
    m.set_wide_rows([77], np.zeros((1, G), dtype=np.uint16))
    rc, message, _ = raw_call(kgx, m, groups, 6, 3, None, L)
    assert rc == kgx.KGX_EINVAL and "locus 77" in message and "wide" in message
    rc, message, _ = raw_call(kgx, m, groups, 6, 3, [3, 77, 80], 3)
    assert rc == kgx.KGX_EINVAL and "locus 77" in message
    rc, _, out = raw_call(kgx, m, groups, 6, 3, [3, 76, 78], 3)              # the wide locus left out: served
    assert rc == kgx.KGX_OK and np.array_equal(out, expected(G, 6, 3)[[3, 76, 78]])
    m.set_wide_rows(None, None)
    rc, _, _ = raw_call(kgx, m, groups, 6, 3, None, L)
    assert rc == kgx.KGX_OK
    m.close()


def test_synthetic_multiallelic_population(kgx):
    """kgx_gt8_synth_multiallelic on the device against the restatement over the host twin's bytes."""
    G, n_loci, seed = 300, 2000, 20261
    m = kgx.GenotypeMatrix(G, n_loci)
    m.synth_multiallelic(seed, 0, 0)
    twin, _, _ = kgx.synth_multiallelic_host(seed, 0, G, 0, n_loci)
    groups = (np.arange(G) % 7).astype(np.uint8)
    groups[groups == 6] = 0xFF
    got = m.allele_census(groups, 6, 3)
    m.close()
    assert np.array_equal(got, acr.census(twin, groups, 6, 3))
    assert got[:, :, 3:].any()
