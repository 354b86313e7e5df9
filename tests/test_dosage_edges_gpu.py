"""The 2-bit dosage sweeps where their counters saturate and their slices repeat.  Needs a real MI355X.

At test sizes the host cuts the work so finely that a lane of k_count_by_genome never fills a carry-save plane above weight
16 nor flushes before its end, a slice of k_compound_offsets / k_offset_filters holds one group, and a slice of
k_genome_row_lists one 64-row tile.  KGX_K3_PIECES / KGX_K8_SLICES / KGX_LIST_SLICES cap the number of pieces, so that these
tests reach at a few MB what a piece does at full size; kgx_dosage_last_work says how the launch was really cut, so that no
test quietly takes the short path.  Every comparison is exact, against plain counting over the codes (tests/dosage_reference.py).
"""
import contextlib
import functools
import time

import numpy as np
import pytest

from . import dosage_reference as ref

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def switches(kgx, monkeypatch, **values):
    for name, value in values.items():
        monkeypatch.setenv(name, str(value))
    kgx.reload_options()
    try:
        yield
    finally:
        for name in values:
            monkeypatch.delenv(name)
        kgx.reload_options()


class Findings:
    """Every comparison of a test is made, then all that differ are reported together."""

    def __init__(self):
        self.bad = []

    def same(self, what, got, want, describe=None):
        want = np.asarray(want).astype(got.dtype)
        if got.shape != want.shape or not np.array_equal(got, want):
            note = describe(got, want) if describe is not None and got.shape == want.shape else ""
            self.bad.append(f"{what}{note}")

    def finish(self):
        assert not self.bad, "\n".join(self.bad)


# ---- K3 across flush periods ---------------------------------------------------------------------------------------------

ROLES = ("zero", "one", "two", "three", "parity", "odd", "first", "tail", "r50", "r80", "r95")
PER_CLASS = 40                     # distinct row patterns per (row parity, region of the list)


def column_group_lasts(pitch, G):
    """The last genome of every column group but the last one (the sweep cuts rows of more than 64 chunks into groups of
    whole 128-byte lines, as equal as that allows)."""
    chunks = pitch // 16
    n_cg = (chunks + 63) // 64
    if n_cg <= 1:
        return []
    width = ((chunks + 7) // 8 + n_cg - 1) // n_cg * 8
    return [min((c + 1) * width * 64, G) - 1 for c in range(n_cg - 1)]


def role_positions(G, group_lasts):
    """genome -> role: the saturated columns at genome 0 and G - 1, on both sides of the dword edge 15 / 16 and the chunk edge
    63 / 64 and of every column-group edge; every role once more inside one dword and near the end."""
    at = {}

    def put(g, role):
        if 0 <= g < G and g not in at:
            at[g] = role

    for g, role in ((0, "three"), (G - 1, "one"), (15, "two"), (16, "one"), (63, "three"), (64, "two")):
        put(g, role)
    for last in group_lasts:
        put(last, "one")
        put(last + 1, "three")
    for g, role in ((1, "zero"), (14, "parity"), (17, "first"), (62, "tail"), (65, "r95"), (G - 2, "two"), (G - 3, "odd")):
        put(g, role)
    for i, role in enumerate(ROLES):
        put(20 + i, role)
        put(G - 40 + i, role)
    assert set(at.values()) == set(ROLES)
    return at


class PatternPopulation:
    """V rows drawn from 6 * PER_CLASS distinct row patterns: a row's pattern comes from the class of its (parity, region)
    -- region 0 = the first flush period, 2 = the last 5 rows (the ragged step), 1 = between -- so that columns with a fixed
    role hold for every row, and every count follows exactly from how often each pattern is used."""

    def __init__(self, kgx, G, V, period, group_lasts, seed):
        rng = np.random.default_rng(seed)
        self.G, self.V = G, V
        n_pat = 6 * PER_CLASS
        cls = np.arange(n_pat) // PER_CLASS
        parity, region = cls // 3, cls % 3
        rate = rng.choice([0.02, 0.3, 0.5, 0.8, 0.95], size=G)
        code = rng.choice(np.array([1, 2, 3], dtype=np.uint8), size=(n_pat, G), p=[0.6, 0.3, 0.1])
        patterns = np.where(rng.random((n_pat, G)) < rate, code, 0).astype(np.uint8)
        self.roles = role_positions(G, group_lasts)
        for g, role in self.roles.items():
            if role in ("zero", "one", "two", "three"):
                column = np.full(n_pat, ("zero", "one", "two", "three").index(role))
            elif role == "parity":
                column = np.where(parity == 0, 1, 2)
            elif role == "odd":
                column = np.where(parity == 1, 3, 0)
            elif role == "first":
                column = np.where(region == 0, 1, 0)
            elif role == "tail":
                column = np.where(region == 2, 2, 0)
            else:
                column = np.where(rng.random(n_pat) < int(role[1:]) / 100.0, code[:, g], 0)
            patterns[:, g] = column
        self.patterns = patterns
        v = np.arange(V)
        row_region = np.where(v < period, 0, np.where(v >= V - 5, 2, 1))
        self.pat_of_row = ((v & 1) * 3 + row_region) * PER_CLASS + rng.integers(0, PER_CLASS, V)
        self.packed = kgx.pack_dosage2(patterns)[self.pat_of_row]
        self.is_code = [(patterns == k).astype(np.int64) for k in range(4)]

    def present(self, keep):
        """Rows that still have a carrier among the kept genomes."""
        return (self.patterns[:, keep.astype(bool)] > 0).any(1)[self.pat_of_row]

    def by_genome(self, selected=None, keep=None):
        """[G][4]: how often each genome holds each code over the selected rows; under a mask the rows without a kept
        carrier are out and the genomes left out read zero."""
        sel = np.ones(self.V, dtype=bool) if selected is None else selected.copy()
        if keep is not None:
            sel &= self.present(keep)
        uses = np.bincount(self.pat_of_row[sel], minlength=len(self.patterns)).astype(np.int64)
        out = np.stack([uses @ self.is_code[k] for k in range(4)], 1)
        if keep is not None:
            out[~keep.astype(bool)] = 0
        return out

    def by_variant(self, keep=None):
        """[V][4]: K2's counts over the (kept) genomes."""
        p = self.patterns if keep is None else self.patterns[:, keep.astype(bool)]
        return ref.counts_by_code(p, 1)[self.pat_of_row]

    def roles_of(self, got, want):
        genomes = np.nonzero((got != want).reshape(self.G, -1).any(1))[0]
        roles = sorted({self.roles.get(int(g), "random") for g in genomes})
        return f": {len(genomes)} genomes differ, roles {roles}, first {genomes[:6].tolist()}"


# G, whole periods k, row pitch, column groups, the flush period P(W) = 1,044,480 / W at this row width.
# The rows are laid out for the period the design states; that the kernel's own constants give the same period is asserted
# through kgx_dosage_last_work AFTER the counts, so that a kernel with another period shows in its arithmetic first.
K3_SHAPES = [(64, 1, 16, 1, 1_044_480), (1000, 1, 256, 1, 65_280), (2500, 2, 640, 1, 16_320), (4099, 1, 1152, 2, 16_320)]


@pytest.mark.parametrize("G,k,pitch,n_groups,period", K3_SHAPES)
def test_by_genome_counters_across_flush_periods(kgx, monkeypatch, G, k, pitch, n_groups, period):
    """One work item (KGX_K3_PIECES=1) walks k whole flush periods, then an odd number of 8-row blocks, then a ragged step, over
    columns that are one code throughout (a stream set in every row: every plane up to weight 2048 fills, and a lost carry at
    the flush in the middle or a wrong period shows) -- identity rows, the gathered path of the bins (8-entry scalar index fetch,
    list length no multiple of 8), under a genome mask, and K2 / the population summary on the same rows.

    Shown once on an MI355X with kBlocksPerFlush set to 1024 in the working tree: all four shapes fail in the comparisons that
    walk the whole list (identity rows, under mask A; at G = 64, 1000, 2500 bin 0 as well), in exactly the columns that are code
    1, 2 or 3 throughout or by row parity (and, with two periods at G = 2500, the dense random ones), while K2 and the small
    fuzz tests of test_parity_gpu.py pass."""
    t0 = time.perf_counter()
    V = k * period + 3 * (period // 510) + 5
    pop = kgx.Population(G, V)
    assert pop.row_pitch == pitch
    lasts = column_group_lasts(pitch, G)
    assert len(lasts) + 1 == n_groups
    case = PatternPopulation(kgx, G, V, period, lasts, seed=G)
    rng = np.random.default_rng(G + 1)
    # three bins and rows in none; bin 0 alone is longer than a period
    bins = np.zeros(V, dtype=np.uint8)
    some = rng.permutation(V)[:77 if (V - 29) % 8 else 78]    # (so that the list's length is no multiple of 8)
    bins[some[:37]], bins[some[37:48]], bins[some[48:]] = 1, 2, 0xFF
    assert (bins == 0).sum() > k * period and (bins != 0xFF).sum() % 8 != 0 and V % 8 != 0
    # mask A keeps the saturated columns and drops the neighbours of the code-1 ones (no row loses its last carrier: the
    # gathered list is all V rows); mask B keeps only columns that carry nothing in some rows, so those rows drop out
    keep_a = (rng.random(G) < 0.7).astype(np.uint8)
    keep_b = np.zeros(G, dtype=np.uint8)
    for g, role in case.roles.items():
        keep_a[g] = 1
        keep_b[g] = role in ("zero", "odd", "first", "tail")
    for g, role in case.roles.items():
        if role == "one":
            keep_a[[n for n in (g - 1, g + 1) if 0 <= n < G and case.roles.get(n) != "one"]] = 0
    dropped = int((~case.present(keep_b)).sum())
    assert case.present(keep_a).all() and 0 < dropped < V

    pop.load_dosage2(case.packed)
    got, work = {}, {}
    try:
        with switches(kgx, monkeypatch, KGX_K3_PIECES=1):
            got["identity"] = pop.count_by_genome()
            work["identity"] = kgx.dosage_last_work("by_genome")
            got["binned"] = pop.count_by_genome_binned(bins, 3)
            work["binned"] = kgx.dosage_last_work("by_genome")
            pop.set_genome_mask(keep_a)
            got["k2 masked"] = pop.allele_count_by_locus()
            got["summary masked"] = pop.population_summary()
            got["masked"] = pop.count_by_genome()
            work["masked"] = kgx.dosage_last_work("by_genome")
            got["masked binned"] = pop.count_by_genome_binned(bins, 3)
            pop.set_genome_mask(keep_b)
            got["rows dropped"] = pop.count_by_genome()
            work["rows dropped"] = kgx.dosage_last_work("by_genome")
            pop.set_genome_mask(None)
        got["uncapped"] = pop.count_by_genome()
        work["uncapped"] = kgx.dosage_last_work("by_genome")
        got["k2"] = pop.allele_count_by_locus()
        got["summary"] = pop.population_summary()
    finally:
        pop.close()
    print(f"by-genome G={G} V={V}: (pieces, longest, period) {work} | {time.perf_counter() - t0:.2f} s")

    f = Findings()
    f.same("identity rows", got["identity"], case.by_genome(), case.roles_of)
    f.same("without the cap", got["uncapped"], case.by_genome(), case.roles_of)
    for b in range(3):
        f.same(f"bin {b}", got["binned"][:, b, :], case.by_genome(bins == b), case.roles_of)
        f.same(f"bin {b} under mask A", got["masked binned"][:, b, :], case.by_genome(bins == b, keep_a), case.roles_of)
    f.same("under mask A", got["masked"], case.by_genome(None, keep_a), case.roles_of)
    f.same("under mask B (rows drop out)", got["rows dropped"], case.by_genome(None, keep_b), case.roles_of)
    f.same("K2", got["k2"], case.by_variant())
    f.same("population summary", got["summary"], case.by_variant().sum(0))
    f.same("K2 under mask A", got["k2 masked"], case.by_variant(keep_a))
    f.same("population summary under mask A", got["summary masked"], case.by_variant(keep_a).sum(0))
    f.finish()
    # the cap is what is being tested: one piece longer than k periods with it, many pieces without
    assert work["identity"] == (1, V, period) and V > k * period
    assert work["binned"] == (1, int((bins != 0xFF).sum()), period)
    assert work["masked"] == (1, V, period)
    assert work["rows dropped"] == (1, V - dropped, period)
    assert work["uncapped"][0] > 1 and work["uncapped"][1] < period


def test_phase_plane_counters_across_a_flush_period(kgx, monkeypatch):
    """The phase plane of 2500 genomes (320-byte rows: 32 lanes per row, 12 of them idle) walked by one work item across a flush
    period, with plane columns set in every row and by row parity: kgx_unique_phased_counts = variants carried + plane bits."""
    t0 = time.perf_counter()
    G, period = 2500, 32_640
    V = period + 3 * (period // 510) + 5
    case = PatternPopulation(kgx, G, V, period, [], seed=77)
    rng = np.random.default_rng(78)
    cls = np.arange(len(case.patterns)) // PER_CLASS
    plane = rng.random(case.patterns.shape) < 0.5
    for g in (0, 15, 16, 127, 128, G - 1):              # set throughout: both sides of the dword and the 128-genome chunk edges
        plane[:, g] = True
    for g in (1, 126, 129, G - 2):                       # by row parity
        plane[:, g] = cls // 3 == g % 2
    plane[:, [2, 130]] = False
    bins = np.zeros(V, dtype=np.uint8)
    some = rng.permutation(V)[:70]
    bins[some[:40]], bins[some[40:]] = 1, 0xFF
    assert (bins == 0).sum() > period

    def want(selected):
        uses = np.bincount(case.pat_of_row[selected], minlength=len(case.patterns)).astype(np.int64)
        return uses @ ((case.patterns > 0).astype(np.int64) + plane)

    pop = kgx.Population(G, V)
    pop.load_dosage2(case.packed)
    pop.load_phase_plane(plane[case.pat_of_row])
    try:
        with switches(kgx, monkeypatch, KGX_K3_PIECES=1):
            got = pop.unique_phased_counts()
            work = kgx.dosage_last_work("by_genome")
            got_binned = pop.unique_phased_counts(bins, 2)
            work_binned = kgx.dosage_last_work("by_genome")
        got_free = pop.unique_phased_counts()
        work_free = kgx.dosage_last_work("by_genome")
    finally:
        pop.close()
    print(f"phase plane G={G} V={V}: (pieces, longest, period) {work} binned {work_binned} uncapped {work_free} | {time.perf_counter() - t0:.2f} s")
    f = Findings()
    f.same("every row", got[:, 0], want(np.ones(V, dtype=bool)))
    f.same("without the cap", got_free[:, 0], want(np.ones(V, dtype=bool)))
    for b in range(2):
        f.same(f"bin {b}", got_binned[:, b], want(bins == b))
    f.finish()
    assert work == (1, V, period) and V > period
    assert work_binned == (1, int((bins != 0xFF).sum()), period)
    assert work_free[0] > 1 and work_free[1] < period


# ---- K8 over many groups per slice ---------------------------------------------------------------------------------------

GROUP_SIZES = (2, 3, 14, 15, 16, 17, 29, 30, 31, 46)       # around one and two and three drains of the 4-bit field sums
OFFSET_BINS = 5
N_GROUPS = 600


@functools.lru_cache(maxsize=None)
def offsets_case(G):
    """~600 compound offsets of the sizes above with single rows between them.  Fixed genomes carry all rows of every group at
    code 1 / 2 / 3, exactly one row, none; every ninth group is carried by nobody; genomes 32..47 (a dword column) carry nothing."""
    rng = np.random.default_rng(1000 + G)
    sizes = np.concatenate([np.array(GROUP_SIZES), rng.choice(GROUP_SIZES, N_GROUPS - len(GROUP_SIZES))])
    rng.shuffle(sizes)
    roles = {}
    for g, role in ((0, "all1"), (1, "all2"), (2, "all3"), (3, "single"), (4, "none"), (15, "all3"), (16, "all1"), (14, "single"), (17, "all2"),
                    (63, "all1"), (64, "all3"), (62, "all2"), (65, "single"), (G - 1, "all2"), (G - 2, "all1"), (G - 3, "all3"), (G - 4, "single"),
                    (G - 5, "none")):
        if 0 <= g < G and g not in roles:
            roles[g] = role
    blocks, groups, singles, row = [], [], [], 0
    for i, n in enumerate(sizes):
        for _ in range(int(rng.integers(0, 3))):           # offsets of one row between the groups
            blocks.append(np.where(rng.random((1, G)) < 0.3, rng.integers(1, 4, (1, G)), 0))
            singles.append(row)
            row += 1
        block = np.where(rng.random((n, G), dtype=np.float32) < rng.choice([0.05, 0.3, 0.7]), rng.choice([1, 2, 3], size=(n, G), p=[0.6, 0.3, 0.1]), 0)
        if i % 9 == 4:
            block[:] = 0
        else:
            block[:, 32:48] = 0
            for g, role in roles.items():
                block[:, g] = {"all1": 1, "all2": 2, "all3": 3}.get(role, 0)
                if role == "single":
                    block[rng.integers(0, n), g] = rng.integers(1, 4)
        blocks.append(block)
        groups.append(np.arange(row, row + n))
        row += n
    codes = np.concatenate(blocks).astype(np.uint8)
    single_bin = np.full(len(codes), 0xFF, dtype=np.uint8)
    single_bin[singles] = np.where(rng.random(len(singles)) < 0.8, rng.integers(0, OFFSET_BINS, len(singles)), 0xFF)
    bins = {"runs": np.sort(rng.integers(0, OFFSET_BINS, N_GROUPS)), "scrambled": rng.integers(0, OFFSET_BINS, N_GROUPS)}
    want = {}
    for order, b in bins.items():
        listed = [(rows, int(bin_)) for rows, bin_ in zip(groups, b)]
        alone = [(np.array([r]), int(single_bin[r])) for r in singles if single_bin[r] != 0xFF]
        want[order] = (ref.compound_offsets(codes, listed, OFFSET_BINS), ref.offset_filter_counts(codes, listed + alone, OFFSET_BINS))
    shuffle = rng.permutation(len(codes))
    return codes, groups, single_bin, bins, want, shuffle


@pytest.mark.parametrize("G,slices,order", [(70, 1, "runs"), (70, 3, "runs"), (4097, 1, "runs"), (4097, 3, "runs"), (4097, 3, "scrambled")])
def test_compound_offsets_over_many_groups_per_slice(kgx, monkeypatch, G, slices, order):
    """KGX_K8_SLICES: a slice of k_compound_offsets / k_offset_filters walks 200 or 600 groups -- the counters carried in
    registers from group to group, flushed where the bin changes inside the slice (runs of bins, as contigs come; once in
    scrambled order), the groups nobody carries skipped -- with the 4-bit field sums at 15, 16, 30, 31 rows and genomes that
    carry every row of a group."""
    t0 = time.perf_counter()
    codes, groups, single_bin, bins, want, shuffle = offsets_case(G)
    want_compound, want_filters = want[order]
    V = len(codes)
    count = np.array([len(rows) for rows in groups], dtype=np.uint32)
    first = np.array([rows[0] for rows in groups], dtype=np.uint32)
    starts = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.uint32)
    members = np.concatenate(groups).astype(np.uint32)
    position = np.empty(V, dtype=np.int64)
    position[shuffle] = np.arange(V)                           # old row r sits at position[r] of the shuffled population
    gbin = bins[order].astype(np.uint32)
    pop, shuffled = kgx.Population(G, V), kgx.Population(G, V)
    pop.load_dosage2(kgx.pack_dosage2(codes))
    shuffled.load_dosage2(kgx.pack_dosage2(codes[shuffle]))
    try:
        with switches(kgx, monkeypatch, KGX_K8_SLICES=slices):
            adjacent = pop.compound_offsets(first, count, gbin, OFFSET_BINS)
            work = kgx.dosage_last_work("offsets")
            listed = shuffled.compound_offsets_listed(position[members].astype(np.uint32), starts, count, gbin, OFFSET_BINS)
            work_listed = kgx.dosage_last_work("offsets")
            filters = pop.offset_filter_counts(single_bin, members, starts, count, gbin, OFFSET_BINS)
            work_filters = kgx.dosage_last_work("offsets")
        free = pop.compound_offsets(first, count, gbin, OFFSET_BINS)
        work_free = kgx.dosage_last_work("offsets")
    finally:
        pop.close()
        shuffled.close()
    print(f"offsets G={G} V={V} {order}: (slices, groups per slice, field rows) {work} uncapped {work_free} | {time.perf_counter() - t0:.2f} s")
    per_slice = -(-N_GROUPS // slices)
    assert work == work_listed == work_filters == (slices, per_slice, 15) and per_slice >= 4
    assert work_free[0] > slices and work_free[1] < per_slice
    f = Findings()
    f.same("adjacent rows", adjacent, want_compound)
    f.same("listed rows", listed, want_compound)
    f.same("without the cap", free, want_compound)
    f.same("offset filters", filters, want_filters)
    f.finish()
    assert want_compound[:, :, 1].max() >= 46 and (want_compound.sum(2) == 0).any()


# ---- row lists over several tiles per slice --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lists_case(G, V):
    """Sparse random codes, and columns of their own: a genome carrying every row; genomes with exactly 0 .. 5 entries; one
    with entries only in the last ragged tile; and at several tile edges e genomes carrying rows e-1 .. e+2, e-2 .. e+1,
    e-3 .. e -- 1, 2, 3 entries waiting for a fourth when the tile ends."""
    rng = np.random.default_rng(G * 10000 + V)
    codes = rng.choice(np.arange(4, dtype=np.uint8), size=(V, G), p=[0.85, 0.1, 0.04, 0.01])
    columns = [1 + np.arange(V) % 3]
    for n in range(6):
        column = np.zeros(V, dtype=np.uint8)
        column[rng.choice(V, n, replace=False)] = rng.integers(1, 4, n)
        columns.append(column)
    column = np.zeros(V, dtype=np.uint8)
    column[V // 64 * 64:] = 2
    columns.append(column)
    for e in (64, 192, 448, 896):
        for before in (1, 2, 3):
            column = np.zeros(V, dtype=np.uint8)
            column[max(0, e - before):min(V, e - before + 4)] = 1
            columns.append(column)
    places = [0, G - 1, 63, 64] + list(range(1, 18))
    if G > 260:
        places += [255, 256, G - 2, 128] + list(range(240, 255))
    places = list(dict.fromkeys(places))                       # (G = 65: genome 64 is the last one)
    special = {}
    for i, g in enumerate(places):
        codes[:, g] = columns[i % len(columns)]
        special[g] = i % len(columns)
    assert len(places) >= len(columns) and len(set(places)) == len(places)
    return codes, special


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("V", [64 * 7 + 1, 64 * 20 + 63])
@pytest.mark.parametrize("G", [65, 257, 4097])
def test_row_lists_over_several_tiles_per_slice(kgx, monkeypatch, G, V, slices):
    """KGX_LIST_SLICES: a slice of k_genome_row_lists walks 3 to 21 tiles of 64 rows, its store queue of up to three row numbers
    carried from tile to tile, and the cursors of a later slice follow a slice of several tiles."""
    t0 = time.perf_counter()
    codes, special = lists_case(G, V)
    rng = np.random.default_rng(5)
    g0, g1 = 3, G - 2
    selected = rng.random(V) < 0.5
    keep = (rng.random(G) < 0.6).astype(np.uint8)
    keep[[g for g in special if g % 3 != 1]] = 1
    pop = kgx.Population(G, V)
    pop.load_dosage2(kgx.pack_dosage2(codes))
    try:
        with switches(kgx, monkeypatch, KGX_LIST_SLICES=slices):
            plain = pop.genome_row_lists()
            work = kgx.dosage_last_work("row_lists")
            ranged = pop.genome_row_lists(g0, g1, selected)
            pop.set_genome_mask(keep)
            masked = pop.genome_row_lists()
            masked_ranged = pop.genome_row_lists(g0, g1, selected)
            pop.set_genome_mask(None)
        free = pop.genome_row_lists()
        work_free = kgx.dosage_last_work("row_lists")
    finally:
        pop.close()
    print(f"row lists G={G} V={V}: (slices, rows per slice, tile rows) {work} uncapped {work_free} | {time.perf_counter() - t0:.2f} s")
    assert work[0] == slices and work[2] == 64 and work[1] >= 3 * work[2] and work[1] * slices >= V
    assert work_free[0] > slices and work_free[1] == work_free[2]
    f = Findings()
    for what, got, want in (("plain", plain, ref.row_lists(codes, 0, G)), ("without the cap", free, ref.row_lists(codes, 0, G)),
                            ("sub-range and selection", ranged, ref.row_lists(codes, g0, g1, selected)),
                            ("genome mask", masked, ref.row_lists(codes, 0, G, None, keep)),
                            ("genome mask, sub-range and selection", masked_ranged, ref.row_lists(codes, g0, g1, selected, keep))):
        f.same(what + ": begin", got[0], want[0])
        f.same(what + ": rows", got[1], want[1])
    f.finish()


# ---- K2 launch flavours ----------------------------------------------------------------------------------------------------

def lanes_per_row(pitch):
    w = 1
    while w < 64 and w < pitch // 16:
        w *= 2
    return w


def by_genome_under(codes, keep=None):
    rows = codes if keep is None else codes[(codes[:, keep.astype(bool)] > 0).any(1)]
    out = ref.counts_by_code(rows, 0)
    if keep is not None:
        out[~keep.astype(bool)] = 0
    return out


@pytest.mark.parametrize("G,align,pitch", [(65, 128, 128), (1000, None, None), (4099, 16, 1040)])
def test_allele_count_launch_flavours(kgx, monkeypatch, G, align, pitch):
    """The K2 launch flavours the tuning switches select -- 1, 2, 4 row sets in flight per wave, plain instead of non-temporal
    loads, a quarter of the covering lanes per row (a lane then walks several chunks of its row) -- and populations created
    under another row pitch (KGX_PITCH_ALIGN): all must count what the default launch counts, masked and unmasked."""
    t0 = time.perf_counter()
    V = 513
    rng = np.random.default_rng(G)
    codes = rng.choice(np.arange(4, dtype=np.uint8), size=(V, G), p=[0.5, 0.25, 0.15, 0.1])
    codes[100], codes[200] = 3, 0
    keep = (rng.random(G) < 0.6).astype(np.uint8)
    want, want_masked = ref.counts_by_code(codes, 1), ref.counts_by_code(codes[:, keep.astype(bool)], 1)
    packed = kgx.pack_dosage2(codes)
    f = Findings()

    def sweep(pop, what):
        f.same(what, pop.allele_count_by_locus(), want)
        pop.set_genome_mask(keep)
        f.same(what + ", masked", pop.allele_count_by_locus(), want_masked)
        pop.set_genome_mask(None)

    pop = kgx.Population(G, V)
    pop.load_dosage2(packed)
    quarter = max(1, lanes_per_row(pop.row_pitch) // 4)
    assert pop.row_pitch // 16 > quarter                      # a lane takes more than one chunk of its row
    try:
        sweep(pop, "default")
        for flavour in ({"KGX_K2_U": 1}, {"KGX_K2_U": 2}, {"KGX_K2_U": 4}, {"KGX_K2_NT": 0}, {"KGX_K2_NT": 0, "KGX_K2_U": 2}, {"KGX_K2_W": quarter},
                        {"KGX_K2_W": quarter, "KGX_K2_U": 1}):
            with switches(kgx, monkeypatch, **flavour):
                sweep(pop, str(flavour))
    finally:
        pop.close()
    if align is not None:
        with switches(kgx, monkeypatch, KGX_PITCH_ALIGN=align):
            again = kgx.Population(G, V)                      # the pitch is decided when the population is created
        try:
            assert again.row_pitch == pitch
            again.load_dosage2(packed)
            sweep(again, f"pitch {pitch}")
            f.same(f"pitch {pitch}: by genome", again.count_by_genome(), by_genome_under(codes))
            again.set_genome_mask(keep)
            f.same(f"pitch {pitch}: by genome, masked", again.count_by_genome(), by_genome_under(codes, keep))
        finally:
            again.close()
    print(f"K2 flavours G={G}: {time.perf_counter() - t0:.2f} s")
    f.finish()
