"""The populations the objective is checked on (tests/test_loglik_reference_cpu.py, tests/test_loglik_objective_gpu.py),
each built once a session: the window population of test_inbreed_window_vs_oracle (repeated records, unknown alts,
offsets with three or more variants, same-phase pairs, missing frequencies), the C5-style synthetic one, and a
constructed one whose table sits on the edges of the arithmetic."""
from __future__ import annotations

import functools

import numpy as np

from . import inbreed_inputs as ii
from . import oracle_api as oa
from . import synth_vcf as sv

WINDOW = dict(lower=200, upper=40_000, spacing=60, min_af=0.02, max_af=0.9)


def build(G, L, mode, seed):
    rec, gt = sv.multiallelic_block(G, L, rng_seed=seed, missing_af_frac=0.03, dup_records=60)   # repeated records: same-phase pairs, >= 3 variants
    ids = sv.genome_ids(G)
    ref = oa.Population("gnomad")
    ref.add_genomes(["Reference"])
    ref.add_records(rec, None, oa.Population.REFERENCE)
    dip = sv.oracle_population(rec, gt, ids, mode)
    return rec, gt, ids, ref.filter_snp_pass(), dip


@functools.lru_cache(maxsize=None)
def window_population(mode):
    """build(101, 1200, mode, seed=5) with what the device and the numpy reference are given of it: bytes [L][G] in the
    caller's genome order, and per super population (ALL, 2) the table and the window's selection."""
    G, L = 101, 1200
    rec, gt, ids, ref, dip = build(G, L, mode, seed=5)
    loci = ii.ReferenceLoci(rec)
    amax = max(len(a) for a in loci.alts)
    phased = mode == oa.Population.PHASED
    rows = ii.encode_gt8(rec, gt, loci, phased_order=phased)
    windows = {}
    for sp in (oa.ALL, 2):
        table = loci.af_table(sp, amax)
        sel = loci.sample(table, WINDOW["lower"], WINDOW["upper"], WINDOW["spacing"], WINDOW["min_af"], WINDOW["max_af"])
        windows[sp] = (table, sel)
    return dict(G=G, n_loci=len(loci.offsets), ref=ref, dip=dip, order=dip.genome_order(), rows=rows, phased=phased, windows=windows)


def oracle_objective(pop, sp, F):
    """logLikelihood of the window population's genomes, oracle's genome order, at F (that order too)."""
    w = WINDOW
    return oa.loglikelihood_at(pop["ref"], pop["dip"], np.full(pop["G"], sp, dtype=np.int32), w["lower"], w["upper"], w["spacing"], w["min_af"],
                               w["max_af"], F)


def oracle_counts(pop, sp):
    w = WINDOW
    counts, _, present, _ = oa.inbreed_window(pop["ref"], pop["dip"], np.full(pop["G"], sp, dtype=np.int32), "Simple", w["lower"], w["upper"],
                                              w["spacing"], 1000, w["min_af"], w["max_af"])
    assert present.all()
    return counts


SYNTH_G, SYNTH_L = 136, 9000


@functools.lru_cache(maxsize=None)
def synth_population():
    """sv.synth_multiallelic_coded(136, 0, 9000) and its oracle populations, as test_iterative_estimators_at_scale_vs_oracle
    makes them: every locus, one window."""
    d = sv.synth_multiallelic_coded(SYNTH_G, 0, SYNTH_L)
    ref = oa.Population("gnomad")
    ref.add_genomes(["Reference"])
    ref.add_records_coded("chr1", d["offsets"], d["ref_code"], d["n_alts"], d["alt_code"], d["af_flat"], None, oa.Population.REFERENCE)
    dip = oa.Population("diploid")
    dip.add_genomes(sv.genome_ids(SYNTH_G))
    dip.add_records_coded("chr1", d["offsets"], d["ref_code"], d["n_alts"], d["alt_code"], d["af_flat"], d["alleles"], oa.Population.PHASED)
    return dict(G=SYNTH_G, ref=ref.filter_snp_pass(), dip=dip, order=dip.genome_order(), rows=d["gt8"], table=d["table"],
                upper=int(d["offsets"][-1]) + 1, phased=True)


def synth_oracle_objective(pop, F):
    return oa.loglikelihood_at(pop["ref"], pop["dip"], np.full(pop["G"], oa.ALL, dtype=np.int32), 0, pop["upper"], 1, 0.0, 1.0, F)


def synth_oracle_counts(pop):
    counts, _, present, _ = oa.inbreed_window(pop["ref"], pop["dip"], np.full(pop["G"], oa.ALL, dtype=np.int32), "Simple", 0, pop["upper"], 1, 10**9,
                                              0.0, 1.0)
    assert present.all()
    return counts


EDGE_G, EDGE_L, EDGE_AMAX = 77, 2600, 6
EDGE_NAMED = (3, 20, 41, 76)            # the genomes with (0, a) cells of an alt at 0.75: 2*f*f > 1/2


@functools.lru_cache(maxsize=None)
def edge_population():
    """The constructed population: 77 genomes x 2600 loci, six alts, phased (seven classes of homozygous cell; the major
    class spans two items of 2048 loci).  Most loci are ordinary (one to six alts between 0.01 and 0.3); the first ~90
    carry the edges, one frequency of interest a locus, in a slot that moves through the six (NaN alts before and between):
      * 2^-k for k = 1..20 and the doubles next to each -- bin edges; 2^-20 is the smallest frequency with a bin, so its lower
        neighbour, a frequency in (0, 2^-20) that would send the whole call to the passes, is left out -- each beside a
        companion alt at 0.125;
      * 0.0 (its own bin; every cell of it on the floor);
      * a major frequency on either side of 0.01, as close as a table gets: p_major = 1 - sum is a multiple of 2^-53, the
        double 0.01 is not, so the two multiples that bracket it (and 0.0100001 / 0.0099999 beside them);
      * sums of 1 + 2e-5 (not valid: nothing counts there) and 1 + 5e-6 (valid, p_major = 0);
      * an alt at 0.75 whose (0, a) cells -- in EDGE_NAMED alone -- have 2*f*f = 1.125.
    Bytes: 0x00 mostly, every kind of carrier, indices 7 and 15, 0xFF, (0, a) pairs where 2*f*f <= 1/2, homozygotes of every
    edge alt (at 2^-20: floored even at F >= 0, y*y < 1e-10).
    `quiet`: the loci without those of 2^-16, 2^-17 and their neighbours.  The (0, a) entry of such an alt has
    2*f*f in [5e-11, 1e-9), which makes it the call's smallest heterozygous product -- carried or not -- and hands every
    genome with heterozygous cells to the passes from F ~ 0.14 (kgx_kernels_loglik.h); over `quiet` the smallest product
    is >= 1.8e-9 and the moments serve every genome but EDGE_NAMED up to F = 0.9."""
    G, L, amax = EDGE_G, EDGE_L, EDGE_AMAX
    rng = np.random.default_rng(20270)
    n_alts = rng.integers(1, amax + 1, L)
    table = np.where(np.arange(amax)[None, :] < n_alts[:, None], rng.uniform(0.01, 0.08, (L, amax)), np.nan)
    table[:, 0] = rng.uniform(0.05, 0.3, L)
    edges = []
    for k in range(1, 21):
        x = 2.0 ** -k
        edges += ([np.nextafter(x, 0.0)] if k < 20 else []) + [x, np.nextafter(x, 1.0)]
    edges.append(0.0)
    n_edge = len(edges)                                                   # 60
    edge_slot = np.arange(n_edge) % amax
    noisy = []
    for i, x in enumerate(edges):
        table[i] = np.nan
        table[i, edge_slot[i]] = x
        table[i, (edge_slot[i] + 2) % amax] = 0.125
        if 5e-11 <= 2.0 * x * x < 1.0000001e-9:
            noisy.append(i)
    at = n_edge
    q = np.floor(0.01 * 2.0 ** 53)
    major_edges = [q * 2.0 ** -53, (q + 1.0) * 2.0 ** -53, 0.0099999, 0.0100001]
    assert major_edges[0] < 0.01 < major_edges[1]
    major_loci = np.arange(at, at + 4)
    for p in major_edges:
        table[at] = np.nan
        table[at, 0] = 1.0 - p
        at += 1
    not_valid, barely_valid = at, at + 1
    table[not_valid] = [0.5, np.nan, 0.25, 0.25 + 2e-5, np.nan, np.nan]
    table[barely_valid] = [0.5, np.nan, 0.25, 0.25 + 5e-6, np.nan, np.nan]
    at += 2
    big_loci = np.arange(at, at + 7)
    table[big_loci] = np.nan
    table[big_loci, 1] = 0.75
    table[big_loci, 4] = 0.125
    at += 7
    table[at] = [0.1, np.nan, 0.05, np.nan, np.nan, 0.02]                 # NaN alts in the middle of a list
    at += 1
    n_special = at

    # bytes: a draw per cell
    present = ~np.isnan(table)
    first = present.argmax(axis=1) + 1                                    # a present alt of every locus ...
    other = amax - present[:, ::-1].argmax(axis=1)                        # ... and its last (the same where there is one)
    kind = rng.random((L, G))
    a = np.where(rng.random((L, G)) < 0.5, first[:, None], other[:, None]).astype(np.uint8)
    b = np.where(a == first[:, None], other[:, None], first[:, None]).astype(np.uint8)
    rows = np.zeros((L, G), dtype=np.uint8)
    rows = np.where((kind >= 0.66) & (kind < 0.80), a, rows)              # major heterozygote
    rows = np.where((kind >= 0.80) & (kind < 0.88), a | (a << 4), rows)   # minor homozygote
    rows = np.where((kind >= 0.88) & (kind < 0.93), a | (b << 4), rows)   # two alts (one alt: the homozygote again)
    rows = np.where((kind >= 0.93) & (kind < 0.96), a << 4, rows)         # (0, a)
    odd = np.array([0x07, 0x70, 0x17, 0x0F, 0xF1, 0xFF, 0x77, 0x3F], dtype=np.uint8)
    rows = np.where(kind >= 0.96, odd[rng.integers(0, len(odd), (L, G))], rows).astype(np.uint8)
    # (0, a) where 2*f*f > 1/2 (0.5's upper neighbour, the 0.99s, 0.75): the named genomes' at the 0.75 loci alone
    f_of_a = np.take_along_axis(np.nan_to_num(table), (a.astype(np.int64) - 1), axis=1)
    too_big = ((rows & 15) == 0) & (rows != 0) & (2.0 * f_of_a * f_of_a > 0.5)
    rows = np.where(too_big, a, rows).astype(np.uint8)
    rows[np.ix_(big_loci, np.array(EDGE_NAMED))] = 0x20                    # (0, 2): the alt at 0.75
    # homozygotes of every edge alt, and of the alts beside 0.01
    for i in range(n_edge):
        code = np.uint8((edge_slot[i] + 1) | ((edge_slot[i] + 1) << 4))
        rows[i, (np.arange(6) * 11 + i) % G] = code
    rows[np.ix_(major_loci, np.arange(0, G, 3))] = 0x00
    rows[np.ix_(major_loci, np.arange(1, G, 9))] = 0x11
    quiet = np.setdiff1d(np.arange(L), np.array(noisy)).astype(np.uint32)
    return dict(G=G, L=L, amax=amax, rows=rows, table=table, phased=True, named=np.array(EDGE_NAMED), quiet=quiet, noisy=np.array(noisy),
                n_special=n_special, major_loci=major_loci, not_valid=not_valid, barely_valid=barely_valid, big_loci=big_loci)
