"""A plain restatement of the per-cell arithmetic under the Loglikelihood and HallME estimators, in numpy: the class
decision of generateFrequencies (kga_analysis_inbreed_freq.cpp:425-583, as classify_pair / classify_cell in
kgx_kernels_inbreed.h state it for a genotype byte), logLikelihood(F) (kga_analysis_inbreed_calc.cpp:94-129) and
processHallME's expectation step (:255-285).  Array operations throughout, one genome a column; every probability in
double, exactly as the reference computes it (so a cell sits on the 1e-10 floor for the same F), every log and every
sum in np.longdouble.  tests/test_loglik_reference_cpu.py pins this file to the oracle; the device is then measured
against it (tests/test_loglik_objective_gpu.py).

rows: uint8 [L][G], a genotype byte a cell (low nibble: 1 + the place of the genome's first SNP variant in the locus's
alt list, high nibble: the second; 15: an alt the list does not hold; 0xFF: three or more variants).
table: float64 [L][amax], the alts' frequencies in list order, NaN = the alt is not in the AlleleFreqVector."""
from __future__ import annotations

import numpy as np

NONE, MAJOR_HOM, MAJOR_HET, MINOR_HOM, MINOR_HET = 0, 1, 2, 3, 4
SMALL_PROB = 1e-10
# kgx_kernels_inbreed.h (kLoglikTinyHet) / kgx_kernels_loglik.h: what the moments' contract says about heterozygous cells
TINY_HET, BIG_HET, FLOOR_MARGIN, ALL_FLOORED = 5e-11, 0.5, 1.0000001e-10, 2e-10


def locus_tables(table):
    """(f [L][amax] clipped to [0, 1], NaN kept; valid [L]; p_major [L]): AlleleFreqVector's clamp, checkValidAlleleVector
    and majorAlleleFrequency -- the sum in list order, in double."""
    table = np.asarray(table, dtype=np.float64)
    present = ~np.isnan(table)
    f = np.where(present, np.clip(table, 0.0, 1.0), np.nan)
    total = np.zeros(table.shape[0], dtype=np.float64)
    for a in range(table.shape[1]):                       # (list order: a column at a time, every locus at once)
        total = total + np.where(present[:, a], f[:, a], 0.0)
    valid = present.any(axis=1) & ~((total - 1.0) > 1.0e-5)
    p_major = np.clip(1.0 - np.clip(total, 0.0, 1.0), 0.0, 1.0)
    return f, valid, p_major


def classify(rows, table, phased):
    """(cls uint8 [L][G], f1, f2 float64 [L][G]): the class of every cell and the two frequencies its probability is
    made of (NaN where the cell has no class)."""
    rows = np.asarray(rows, dtype=np.uint8)
    f, valid, p_major = locus_tables(table)
    L, amax = f.shape
    assert rows.shape[0] == L
    a1 = (rows & 15).astype(np.int64)
    a2 = (rows >> 4).astype(np.int64)
    usable = valid[:, None] & (a1 != 15) & (a2 != 15) & (a1 <= amax) & (a2 <= amax)
    padded = np.concatenate([np.full((L, 1), np.nan), f], axis=1)            # index 0: no allele
    fa1 = np.take_along_axis(padded, np.minimum(a1, amax), axis=1)
    fa2 = np.take_along_axis(padded, np.minimum(a2, amax), axis=1)
    has1, has2 = ~np.isnan(fa1), ~np.isnan(fa2)
    major = np.broadcast_to(p_major[:, None], rows.shape)
    major_hom = usable & (a1 == 0) & (a2 == 0) & (major > 0.01)
    same_phase = usable & (a1 == 0) & (a2 != 0) & has2                       # (0, a): alt a twice on one phase
    major_het = usable & (a1 != 0) & (a2 == 0) & has1
    minor_hom = usable & (a1 != 0) & (a1 == a2) & has1 & bool(phased)
    minor_het = usable & (a1 != 0) & (a2 != 0) & has1 & has2 & ~minor_hom
    cls = np.zeros(rows.shape, dtype=np.uint8)
    cls[major_hom], cls[major_het], cls[minor_hom], cls[minor_het | same_phase] = MAJOR_HOM, MAJOR_HET, MINOR_HOM, MINOR_HET
    f1 = np.full(rows.shape, np.nan)
    f2 = np.full(rows.shape, np.nan)
    f1[major_hom] = f2[major_hom] = major[major_hom]
    f1[same_phase] = f2[same_phase] = fa2[same_phase]
    f1[major_het], f2[major_het] = fa1[major_het], major[major_het]
    f1[minor_hom] = f2[minor_hom] = fa1[minor_hom]
    f1[minor_het], f2[minor_het] = fa1[minor_het], fa2[minor_het]
    return cls, f1, f2


def class_counts(cls):
    """uint64 [G][5] in the oracle's column order: major het, minor het, minor hom, major hom, all four."""
    columns = [(cls == MAJOR_HET), (cls == MINOR_HET), (cls == MINOR_HOM), (cls == MAJOR_HOM), (cls != NONE)]
    return np.stack([c.sum(axis=0) for c in columns], axis=1).astype(np.uint64)


def probabilities(cells, F):
    """float64 [L][G]: every cell's clamped probability at its genome's F (1 where the cell has no class), in the
    reference's own double operations."""
    cls, f1, f2 = cells
    F = np.asarray(F, dtype=np.float64)[None, :]
    hom = (cls == MAJOR_HOM) | (cls == MINOR_HOM)
    het = (cls == MAJOR_HET) | (cls == MINOR_HET)
    with np.errstate(invalid="ignore"):
        p_hom = (F * f1) + ((1.0 - F) * (f1 * f1))
        p_het = 2 * (1.0 - F) * f1 * f2
    p = np.where(hom, p_hom, np.where(het, p_het, 1.0))
    return np.clip(p, SMALL_PROB, 1.0)


def loglikelihood(rows, table, phased, F, cells=None):
    """(value, sum of |log p|), np.longdouble [G]: logLikelihood of genome g at F[g].  cells: classify()'s result for
    the same rows and table, where a caller evaluates many points."""
    cells = classify(rows, table, phased) if cells is None else cells
    logs = np.log(probabilities(cells, F).astype(np.longdouble))
    return logs.sum(axis=0), np.abs(logs).sum(axis=0)


def hall_me(rows, table, phased, start, steps=50, cells=None):
    """np.longdouble [G]: `steps` expectation steps of processHallME from start[g]."""
    cls, f1, _ = classify(rows, table, phased) if cells is None else cells
    hom = (cls == MAJOR_HOM) | (cls == MINOR_HOM)
    y = np.where(hom, f1, 1.0).astype(np.longdouble)
    n_cells = (cls != NONE).sum(axis=0).astype(np.longdouble)
    F = np.asarray(start, dtype=np.longdouble).copy()
    zero, one = np.longdouble(0), np.longdouble(1)
    for _ in range(steps):
        denominator = F[None, :] + (one - F[None, :]) * y
        with np.errstate(divide="ignore", invalid="ignore"):
            term = np.where(hom & (denominator != zero), F[None, :] / denominator, zero)
            F = term.sum(axis=0) / n_cells
    return F


def het_products(rows, table, phased, at_least=None, at_most=None, cells=None):
    """(smallest, largest) float64 [G]: 2*f1*f2 over the genome's heterozygous cells (those with at_least <= 2*f1*f2 <=
    at_most where given); +inf / -inf for a genome without one."""
    cls, f1, f2 = classify(rows, table, phased) if cells is None else cells
    keep = (cls == MAJOR_HET) | (cls == MINOR_HET)
    with np.errstate(invalid="ignore"):
        w = 2.0 * f1 * f2
        if at_least is not None:
            keep = keep & (w >= at_least)
        if at_most is not None:
            keep = keep & (w <= at_most)
    return np.where(keep, w, np.inf).min(axis=0, initial=np.inf), np.where(keep, w, -np.inf).max(axis=0, initial=-np.inf)


def kinks(rows, table, phased, cells=None):
    """float64 [L][G]: -y / (1 - y) of every homozygous cell whose kink lies in the optimiser's box (0 < y <= 1/2: below
    that F the cell's probability F*y + (1-F)*y*y is negative, i.e. on the floor); NaN elsewhere."""
    cls, f1, _ = classify(rows, table, phased) if cells is None else cells
    hom = ((cls == MAJOR_HOM) | (cls == MINOR_HOM)) & (f1 > 0.0) & (f1 <= 0.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(hom, -f1 / (1.0 - f1), np.nan)


def median_kink(rows, table, phased, cells=None, fallback=-0.25):
    """float64 [G]: the genome's median kink -- one of its kinks, the lower of the two middle ones -- or `fallback`."""
    k = np.sort(kinks(rows, table, phased, cells=cells), axis=0)              # NaN last
    n = (~np.isnan(k)).sum(axis=0)
    middle = np.take_along_axis(k, np.maximum(n - 1, 0)[None, :] // 2, axis=0)[0]
    return np.where(n > 0, middle, fallback)


def tabulated_het_floor(table, phased):
    """The smallest 2*f1*f2 in [TINY_HET, BIG_HET] over every heterozygous index pair the table can express, carried by a
    genome or not (1.0 where there is none): `the call's smallest w` of kgx_kernels_loglik.h, which the table passes'
    entries are searched for (k_eval_entries<5>)."""
    amax = np.asarray(table).shape[1]
    a1, a2 = np.meshgrid(np.arange(amax + 1), np.arange(amax + 1), indexing="ij")
    pairs = (a1 | (a2 << 4)).astype(np.uint8).ravel()
    every = np.broadcast_to(pairs[None, :], (np.asarray(table).shape[0], pairs.size))
    smallest, _ = het_products(every, table, phased, at_least=TINY_HET, at_most=BIG_HET)
    return float(min(1.0, smallest.min(initial=1.0)))


def served_by_moments(rows, table, phased, F, cells=None):
    """bool [G]: the contract of the objective by moments (kgx_kernels_loglik.h, k_loglik_search), from the reference's
    side.  A genome is handed to the passes -- NaN from the diagnostic -- iff it has a heterozygous cell with
    2*f1*f2 > 1/2 (the clamp's upper bound can bind), or it has heterozygous cells with a term (TINY_HET <= w <= 1/2) and
    (1 - F) * w lies under the floor for the call's smallest such w while not for all of them ((1 - F) > 2e-10)."""
    cells = classify(rows, table, phased) if cells is None else cells
    _, largest = het_products(rows, table, phased, cells=cells)
    with_term, _ = het_products(rows, table, phased, at_least=TINY_HET, at_most=BIG_HET, cells=cells)
    u = 1.0 - np.asarray(F, dtype=np.float64)
    floor_ok = ~np.isfinite(with_term) | (u * tabulated_het_floor(table, phased) >= FLOOR_MARGIN) | (u <= ALL_FLOORED)
    return ~(largest > BIG_HET) & floor_ok


def point_sets(n, kink, seed=2027):
    """The sets of points, one F a genome: P1 the box, P2 the kink-ridden negative side, P3 both bounds, P4 zero, P5
    the genome's median kink, P6 / P7 the doubles next to it, P8 / P9 next to the bounds; P10 next to zero from above,
    10^-k: a homozygous cell of a rare allele (y < 1e-10 / F) is on the floor there, on the side of 0 where the floor's
    root is computed by another branch than at F <= 0 (kgx_kernels_loglik.h: band_of) -- no other set has a point in
    (0, 1e-4), and a build without the floor for F > 0 passed P1..P9."""
    rng = np.random.default_rng(seed)
    g = np.arange(n)
    k = np.array([3, 6, 7, 9, 12])[g % 5]
    kink = np.asarray(kink, dtype=np.float64)
    assert kink.shape == (n,) and np.all((kink >= -1.0) & (kink <= 0.0))
    return {
        "P1": rng.uniform(-1.0, 1.0, n),
        "P2": rng.uniform(-0.6, 0.05, n),
        "P3": np.where(g % 2 == 0, -1.0, 1.0),
        "P4": np.zeros(n),
        "P5": kink.copy(),
        "P6": np.maximum(np.nextafter(kink, -np.inf), -1.0),
        "P7": np.nextafter(kink, np.inf),
        "P8": 1.0 - 10.0 ** -k.astype(np.float64),
        "P9": -1.0 + 10.0 ** -k.astype(np.float64),
        "P10": 10.0 ** -(k + 2).astype(np.float64),
    }
