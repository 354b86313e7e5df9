"""A NumPy restatement of kgx_gt8_allele_census / kgx_census_allele_frequencies (include/kgx.h), the checker of the device census.

A cell of the genotype matrix is one byte: low nibble lo = the first SNP variant the genome carries at the locus, high nibble hi
= the second; 0 = none; 1..14 = 1 + the alt's index in the locus's reference list; 15 = an alt the list does not hold; the byte
0xFF = three or more variants (crowded: nothing is counted from it).  The copies of a cell that is not crowded:
    hi == 0:              lo once
    lo == 0 and hi != 0:  hi TWICE (a repeated record on one phase)
    otherwise:            lo once and hi once (lo == hi: that alt twice)
and per (locus, group) the census holds
    [0] reference_cells  (byte 0x00)        [1] unknown_copies (copies of index 15 or of an index past amax)
    [2] crowded_cells    (byte 0xFF)        [3 + 2 (a - 1)] cells with ONE copy of alt a    [4 + 2 (a - 1)] cells with TWO.
"""
import numpy as np

NO_GROUP = 0xFF


def kinds(amax):
    return 3 + 2 * amax


def cell_copies(cells):
    """copies[..., x] = how many copies of allele index x (0..15) each cell holds; crowded cells hold none; index 0 is never counted."""
    cells = np.asarray(cells, dtype=np.uint8)
    lo, hi = cells & 15, cells >> 4
    crowded = cells == 0xFF
    copies = np.zeros(cells.shape + (16,), dtype=np.uint8)
    index = np.arange(16)
    first = (lo[..., None] == index) & (lo[..., None] != 0) & ~crowded[..., None]
    second = (hi[..., None] == index) & (hi[..., None] != 0) & ~crowded[..., None]
    copies += first
    copies += second
    copies += second & (lo[..., None] == 0)                   # (0, a): that alt twice
    return copies


def census(cells, group_of_genome, n_groups, amax):
    """cells uint8 [L][G], group_of_genome uint8 [G] (a group or 0xFF) -> uint32 [L][n_groups][3 + 2 amax]."""
    cells = np.asarray(cells, dtype=np.uint8)
    groups = np.asarray(group_of_genome, dtype=np.uint8)
    L, G = cells.shape
    assert groups.shape == (G,)
    copies = cell_copies(cells)                                # [L][G][16]
    per_cell = np.zeros((L, G, kinds(amax)), dtype=np.uint8)     # 0, 1 or 2
    per_cell[..., 0] = cells == 0x00
    per_cell[..., 1] = copies[..., amax + 1:].sum(-1, dtype=np.uint8)
    per_cell[..., 2] = cells == 0xFF
    for a in range(1, amax + 1):
        per_cell[..., 3 + 2 * (a - 1)] = copies[..., a] == 1
        per_cell[..., 4 + 2 * (a - 1)] = copies[..., a] == 2
    out = np.zeros((L, n_groups, kinds(amax)), dtype=np.uint32)
    for g in range(n_groups):
        out[:, g, :] = per_cell[:, groups == g, :].sum(1, dtype=np.uint32)
    return out


def group_sizes(group_of_genome, n_groups):
    groups = np.asarray(group_of_genome, dtype=np.uint8)
    return np.array([(groups == g).sum() for g in range(n_groups)], dtype=np.uint64)


def allele_frequencies(census_words, group_genomes, pool, n_alt=None):
    """float64(float32(AC / AN)) [L][amax] over the pooled groups; NaN past n_alt[l] and everywhere when AN == 0."""
    c = np.asarray(census_words, dtype=np.uint64)
    L, _, k = c.shape
    amax = (k - 3) // 2
    pool = [int(p) for p in pool]
    an = 2 * sum(int(group_genomes[p]) for p in pool)
    out = np.full((L, amax), np.nan, dtype=np.float64)
    if an == 0:
        return out
    pooled = c[:, pool, :].sum(1) if pool else np.zeros((L, k), dtype=np.uint64)
    ac = pooled[:, 3::2] + 2 * pooled[:, 4::2]                 # [L][amax]
    af = np.float32(np.float64(ac) / np.float64(an)).astype(np.float64)
    alts = np.full(L, amax) if n_alt is None else np.minimum(np.asarray(n_alt, dtype=np.int64), amax)
    present = np.arange(amax)[None, :] < alts[:, None]
    out[present] = af[present]
    return out
