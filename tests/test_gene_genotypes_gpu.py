"""kgx_gene_genotypes on the device against a NumPy restatement, bit for bit.

The checker restates the reference (kga_analytic/kga_PfEMP/kga_analysis_PfEMP_variant.cpp): a genome CARRIES a row when its
code is not 0; the genotype hash of a (gene, genome) is the sum of the keys of the gene's rows the genome carries, in uint64 (the
sum wraps: the reference adds in size_t); a genome carrying none of the gene's rows is zero-variant, every other genome has a
genotype -- also when its hash is 0; the census is np.unique(..., return_counts=True) of those hashes.

Populations are built cell by cell (V = 4 000 rows, about 200 genes, G in {37, 257, 1000}: a column tail of 5 genomes, more than
one 64-genome chunk, several shards), mostly reference-homozygous with whole all-zero stretches, and carry the special cells the
semantics hinge on: see `build_case`.
"""
import ctypes as C
import zlib
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = 4000
RESERVED = 100          # rows [0, RESERVED) are placed by hand; the random genes draw from the rest
ALL_ONES = 0xFFFFFFFFFFFFFFFF
LOW_ONES = 0x00000000FFFFFFFF


@lru_cache(maxsize=None)
def build_case(G):
    """codes [V][G] uint8, key [V] uint64, genes (list of row arrays), names (gene index by what it is there for)."""
    rng = np.random.default_rng(1000 + G)
    codes = rng.choice(4, size=(V, G), p=[0.90, 0.06, 0.035, 0.005]).astype(np.uint8)
    codes[1000:1400] = 0                                   # a stretch nobody carries anything in: the zero-skip
    codes[:, G // 2:G // 2 + 8][2000:3000] = 0             # ... and dwords that are empty for many rows
    codes[:RESERVED] = 0
    key = rng.integers(0, 2**64, V, dtype=np.uint64)       # the full 64 bits: carries cross bit 32, sums wrap
    genes, names = [], {}

    def add(name, rows):
        names[name] = len(genes)
        genes.append(np.asarray(rows, dtype=np.uint32))

    free = np.arange(RESERVED, V)
    add("no rows", [])
    add("one row", [rng.choice(free)])
    first, last = 0, G - 1                                  # genomes that carry EVERY row of the sized genes
    for n in (15, 16, 17, 300):                             # the 4-bit-field drain boundary; counts past 255
        rows = rng.choice(free[(free < 1000) | (free >= 1400)], n, replace=False)    # unsorted, not adjacent
        add(f"{n} rows", rows)
        codes[rows, first] = 1 + (np.arange(n) % 3).astype(np.uint8)                 # codes 1, 2, 3 in turn
        codes[rows, last] = 2
    big = genes[names["300 rows"]]
    key[big[0]], key[big[1]] = ALL_ONES, LOW_ONES
    shared = rng.choice(free, 30, replace=False)
    add("shares rows a", shared[:20])
    add("shares rows b", shared[10:])
    add("nobody carries", [3, 1, 2])                        # reserved rows left at zero
    # a genome carrying exactly two rows whose keys are k and 2^64 - k: a genotype with hash 0
    k = np.uint64(0x9E3779B97F4A7C15)
    key[10], key[11] = k, np.uint64(2**64 - int(k))
    codes[10, 1 % G] = 1
    codes[11, 1 % G] = 2
    codes[10, 4 % G] = 1                                    # and one genome carrying only the first of them
    add("hash zero", [11, 10])
    # keys 1, 2, 3: {1, 2} and {3} collide into one genotype of two genomes
    key[20], key[21], key[22] = 1, 2, 3
    codes[20, 2 % G] = codes[21, 2 % G] = 1
    codes[22, 3 % G] = 1
    add("collision", [20, 21, 22])
    # code-3 cells
    codes[30, 5 % G] = 3
    codes[31, 5 % G] = 3
    codes[31, 6 % G] = 2
    codes[32, 7 % G] = 1
    add("non diploid", [30, 31, 32])
    # singleton rows: 40 carried by genome 8 alone; 41 and 42 both by genome 9 alone; 43 by three genomes
    codes[40, 8 % G] = 1
    codes[41, 9 % G] = 1
    codes[42, 9 % G] = 2
    codes[43, [9 % G, 10 % G, 11 % G]] = 1
    add("one singleton", [40])
    add("two singletons one genome", [43, 42, 41])
    while len(genes) < 200:
        add(f"random {len(genes)}", rng.choice(free, int(rng.integers(1, 40)), replace=False))
    codes.setflags(write=False)
    key.setflags(write=False)
    return codes, key, genes, names


def row_lists(genes):
    members = np.concatenate(genes).astype(np.uint32)
    n_rows = np.array([len(g) for g in genes], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum(n_rows)[:-1]]).astype(np.uint32)
    return members, first, n_rows


def restate(kgx, codes, key, genes, keep=None):
    """The NumPy restatement: (census, run_begin, run_hash, run_count, hash, counts) as the device must return them."""
    G = codes.shape[1]
    keep = np.ones(G, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    carried = (codes != 0) & keep[None, :]
    carriers = carried.sum(1)
    census = np.zeros(len(genes), dtype=kgx.GENE_CENSUS)
    hashes = np.zeros((len(genes), G), dtype=np.uint64)
    counts = np.zeros((len(genes), G, 4), dtype=np.uint32)
    run_begin, run_hash, run_count = [0], [], []
    for i, rows in enumerate(genes):
        c = carried[rows]                                                        # [n][G]
        hashes[i] = (c * key[rows][:, None]).sum(axis=0, dtype=np.uint64)        # wraps: the reference's size_t sum
        twice = (codes[rows] == 2) & c
        more = (codes[rows] == 3) & c
        single = carriers[rows] == 1
        counts[i, :, 0] = c.sum(0)
        counts[i, :, 1] = twice.sum(0)
        counts[i, :, 2] = more.sum(0)
        counts[i, :, 3] = c[single].sum(0)
        has = counts[i, :, 0] > 0                                                # never hash != 0
        values, sizes = np.unique(hashes[i][has], return_counts=True)
        run_hash.append(values)
        run_count.append(sizes)
        run_begin.append(run_begin[-1] + len(values))
        top = np.zeros(5, dtype=np.uint64)
        biggest = np.sort(sizes)[::-1][:5]
        top[:len(biggest)] = biggest
        census[i] = (keep.sum(), (keep & ~has).sum(), len(values), (c & ~twice & ~more).sum() + 2 * twice.sum(), more.sum(), (carriers[rows] > 0).sum(),
                     single.sum(), (counts[i, :, 3] > 0).sum(), top)
    return (census, np.array(run_begin, dtype=np.uint64), np.concatenate(run_hash).astype(np.uint64), np.concatenate(run_count).astype(np.uint32),
            hashes, counts)


def device_tables(kgx, codes, key, genes, keep=None, **kwargs):
    G = codes.shape[1]
    pop = kgx.Population(G, V)
    pop.load_dosage2(kgx.pack_dosage2(codes))
    if keep is not None:
        pop.set_genome_mask(keep)
    census, (begin, run_hash, run_count), hashes, counts = pop.gene_genotypes(key, *row_lists(genes), **kwargs)
    pop.close()
    return census, begin, run_hash, run_count, hashes, counts


def assert_same(got, want):
    for name, g, w in zip(("census", "run_begin", "run_hash", "run_count", "hash", "counts"), got, want):
        if name == "census":
            for field in w.dtype.names:
                assert np.array_equal(g[field], w[field]), (field, np.flatnonzero((g[field] != w[field]).reshape(len(w), -1).any(1))[:10])
        else:
            assert g.dtype == w.dtype and np.array_equal(g, w), name


@pytest.fixture
def rebind(kgx):
    yield kgx.init
    kgx.init(0)


@lru_cache(maxsize=None)
def expected(G, masked):
    from kgl_gene_amd import capi
    codes, key, genes, _ = build_case(G)
    return restate(capi, codes, key, genes, mask_of(G) if masked else None)


def mask_of(G):
    keep = (np.arange(G) % 3 != 0).astype(np.uint8)         # drops genome 9: the carrier of two singleton rows
    return keep


@pytest.mark.parametrize("G", [37, 257, 1000])
def test_tables_equal_the_numpy_restatement(kgx, G):
    codes, key, genes, names = build_case(G)
    want = expected(G, False)
    got = device_tables(kgx, codes, key, genes)
    assert_same(got, want)
    census, begin, run_hash, run_count, hashes, counts = got
    # the special cells, spelled out (they hold in the restatement too; this pins what they are there for)
    c = census[names["no rows"]]
    assert c["genotypes"] == 0 and c["zero_variant_genomes"] == G and c["unique_variants"] == 0 and not c["top"].any()
    c = census[names["nobody carries"]]
    assert c["genotypes"] == 0 and c["zero_variant_genomes"] == G and c["genomes"] == G
    i = names["hash zero"]
    assert hashes[i, 1 % G] == 0 and counts[i, 1 % G, 0] == 2                   # a genotype, not a zero-variant genome
    assert census[i]["genotypes"] == 2 and census[i]["zero_variant_genomes"] == G - 2
    assert run_hash[int(begin[i])] == 0 and run_count[int(begin[i])] == 1
    i = names["collision"]
    assert census[i]["genotypes"] == 1 and census[i]["top"].tolist() == [2, 0, 0, 0, 0] and hashes[i, 2 % G] == hashes[i, 3 % G] == 3
    i = names["non diploid"]
    assert census[i]["non_diploid_cells"] == 2 and census[i]["variant_objects"] == 3 and census[i]["unique_variants"] == 3
    assert census[names["one singleton"]]["singleton_variants"] == 1 and census[names["one singleton"]]["singleton_genomes"] == 1
    i = names["two singletons one genome"]
    assert census[i]["singleton_variants"] == 2 and census[i]["singleton_genomes"] == 1 and counts[i, 9 % G, 3] == 2
    for n in (15, 16, 17, 300):
        i = names[f"{n} rows"]
        assert counts[i, 0, 0] == n and counts[i, G - 1].tolist()[:3] == [n, n, 0]
    assert (counts[names["300 rows"], :, 0] > 255).any()


@pytest.mark.parametrize("G", [37, 257, 1000])
def test_genome_mask(kgx, G):
    codes, key, genes, names = build_case(G)
    keep = mask_of(G)
    want = expected(G, True)
    got = device_tables(kgx, codes, key, genes, keep=keep)
    assert_same(got, want)
    census, _, _, _, hashes, counts = got
    assert census["genomes"].tolist() == [int(keep.sum())] * len(genes)
    assert not hashes[:, keep == 0].any() and not counts[:, keep == 0].any()
    i = names["two singletons one genome"]                  # their one carrier is masked out: nobody carries them now
    assert census[i]["singleton_variants"] == 0 and census[i]["singleton_genomes"] == 0 and census[i]["unique_variants"] == 1


@pytest.mark.parametrize("G", [37, 257, 1000])
def test_one_device_listed_three_times_gives_identical_results(kgx, rebind, G):
    codes, key, genes, _ = build_case(G)
    rebind([0, 0, 0])
    pop = kgx.Population(G, V)
    n_shards = len([s for s in pop.shards if s["n_genomes"]])
    pop.close()
    assert n_shards == min(3, (G + 63) // 64)
    assert_same(device_tables(kgx, codes, key, genes), expected(G, False))
    assert_same(device_tables(kgx, codes, key, genes, keep=mask_of(G)), expected(G, True))


@pytest.mark.parametrize("small", ["1", "7,3", "64", "1000,16"])
def test_small_slices_and_batches_change_nothing(kgx, monkeypatch, small):
    """KGX_GENE_SMALL=b[,s]: b genes per batch, s (default b) per workgroup slice.  Without it these 200 genes are one batch of
    one-gene slices; with it: a batch per gene; batches of 7 in slices of 3, 3, 1; batches of 64 (the last one of 8) each walked
    by ONE workgroup row; one batch in slices of 16 (the last one of 8)."""
    G = 257
    codes, key, genes, _ = build_case(G)
    monkeypatch.setenv("KGX_GENE_SMALL", small)
    kgx.reload_options()
    try:
        got = device_tables(kgx, codes, key, genes)
        got_masked = device_tables(kgx, codes, key, genes, keep=mask_of(G))
    finally:
        monkeypatch.delenv("KGX_GENE_SMALL")
        kgx.reload_options()
    assert_same(got, expected(G, False))
    assert_same(got_masked, expected(G, True))


def test_hash_and_counts_are_optional(kgx):
    codes, key, genes, _ = build_case(37)
    want = expected(37, False)
    got = device_tables(kgx, codes, key, genes, want_hash=False, want_counts=False)
    assert got[4] is None and got[5] is None
    assert_same(got[:4], want[:4])


def raw_call(kgx, pop, key, genes, run_hash, run_count, capacity):
    members, first, n_rows = row_lists(genes)
    census = np.zeros(len(genes), dtype=kgx.GENE_CENSUS)
    begin = np.zeros(len(genes) + 1, dtype=np.uint64)
    rc = kgx.lib().kgx_gene_genotypes(pop.handle, kgx.ptr(key), kgx.ptr(members), len(members), kgx.ptr(first), kgx.ptr(n_rows), len(genes), None, None,
                                      kgx.ptr(census), kgx.ptr(begin), None if run_hash is None else kgx.ptr(run_hash),
                                      None if run_count is None else kgx.ptr(run_count), capacity)
    return rc, census, begin


def test_sizing_call_and_capacity(kgx):
    G = 257
    codes, key, genes, _ = build_case(G)
    want = expected(G, False)
    pop = kgx.Population(G, V)
    pop.load_dosage2(kgx.pack_dosage2(codes))
    rc, census, begin = raw_call(kgx, pop, key, genes, None, None, 0)
    assert rc == kgx.KGX_OK
    assert_same((census, begin), want[:2])                  # the sizing call fills census and run_begin, top[5] included
    capacity = int(begin[-1])
    assert capacity == len(want[2]) > 0
    run_hash, run_count = np.zeros(capacity, dtype=np.uint64), np.zeros(capacity, dtype=np.uint32)
    rc, census, begin = raw_call(kgx, pop, key, genes, run_hash, run_count, capacity)
    assert rc == kgx.KGX_OK
    assert_same((census, begin, run_hash, run_count), want[:4])
    rc, _, _ = raw_call(kgx, pop, key, genes, run_hash, run_count, capacity - 1)
    assert rc == kgx.KGX_EINVAL and b"capacity" in kgx.lib().kgx_last_error()
    rc, _, _ = raw_call(kgx, pop, key, genes, run_hash, None, capacity)          # one of the two run arrays alone
    assert rc == kgx.KGX_EINVAL
    pop.close()


def test_invalid_row_lists_are_refused(kgx):
    G = 37
    codes, key, genes, _ = build_case(G)
    pop = kgx.Population(G, V)
    pop.load_dosage2(kgx.pack_dosage2(codes))
    with pytest.raises(kgx.KgxError, match="more than once") as err:
        pop.gene_genotypes(key, *row_lists([np.array([5, 9, 5], dtype=np.uint32)]))
    assert err.value.code == kgx.KGX_EINVAL
    with pytest.raises(kgx.KgxError, match="past the population") as err:
        pop.gene_genotypes(key, *row_lists([np.array([1, 2], dtype=np.uint32), np.array([V], dtype=np.uint32)]))
    assert err.value.code == kgx.KGX_EINVAL
    # the same row in two DIFFERENT genes is fine
    census, _, _, _ = pop.gene_genotypes(key, *row_lists([np.array([5, 9], dtype=np.uint32), np.array([9, 5], dtype=np.uint32)]))
    assert len(census) == 2
    members = np.array([1, 2], dtype=np.uint32)
    with pytest.raises(kgx.KgxError) as err:                # a gene reaching past the member list
        pop.gene_genotypes(key, members, np.array([1], dtype=np.uint32), np.array([2], dtype=np.uint32))
    assert err.value.code == kgx.KGX_EINVAL
    census, begin = np.zeros(1, dtype=kgx.GENE_CENSUS), np.zeros(2, dtype=np.uint64)
    none, zero = np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    rc = kgx.lib().kgx_gene_genotypes(pop.handle, None, kgx.ptr(none), 0, kgx.ptr(zero), kgx.ptr(zero), 1, None, None, kgx.ptr(census), kgx.ptr(begin),
                                      None, None, 0)                              # no keys, even for a gene without rows
    assert rc == kgx.KGX_EINVAL and b"null" in kgx.lib().kgx_last_error()
    pop.close()


def test_synthetic_population_read_back(kgx):
    """The device's own generator (dense: AF in [0.01, 0.5]), codes read back from the device for the checker."""
    G = 257
    pop = kgx.Population(G, V)
    pop.synth_biallelic(4242, 0, 0)
    codes = kgx.unpack_dosage2(pop.read_dosage2(), G)
    _, key, genes, _ = build_case(G)
    census, (begin, run_hash, run_count), hashes, counts = pop.gene_genotypes(key, *row_lists(genes))
    pop.close()
    assert_same((census, begin, run_hash, run_count, hashes, counts), restate(kgx, codes, key, genes))
    assert kgx.gene_genotypes_last_ms() > 0.0


def python_gene_csv(kgx, codes, hgvs, genes, ids, coding_length, detail):
    """writeGeneResults (_variant.cpp:109-233) restated: std::ofstream's default formatting of a double is '%g'."""
    key = np.array([zlib.crc32(h.encode()) for h in hgvs], dtype=np.uint64)
    census, begin, _, run_count, _, _ = restate(kgx, codes, key, genes)
    lines = ["Gene_ID,Coding Length,Variant Count,Variant Rate,Unique filter,Unique Variant Rate,Single Genome filter,Single Variant Genomes,"
             "No Variant Genomes,Genotypes,Gini,HRel,2-IQV,Top1 Genotype,Top2 Genotype,Top3 Genotype,Top4 Genotype,Top5 Genotype,Gene Detail"]
    for i in range(len(genes)):
        c = census[i]
        length = int(coding_length[i])
        rate = float(c["variant_objects"]) / length if length else 0.0
        unique_rate = float(c["unique_variants"]) / length if length else 0.0
        gini, hrel, iqv = kgx.genotype_statistics(run_count[int(begin[i]):int(begin[i + 1])], int(c["zero_variant_genomes"]))
        fields = [ids[i], str(length), str(int(c["variant_objects"])), "%g" % rate, str(int(c["unique_variants"])), "%g" % unique_rate,
                  str(int(c["singleton_variants"])), str(int(c["singleton_genomes"])), str(int(c["zero_variant_genomes"])), str(int(c["genotypes"])),
                  "%g" % gini, "%g" % hrel, "%g" % (2.0 - iqv)] + [str(int(t)) for t in c["top"]] + [detail[i]]
        lines.append(",".join(fields))
    return lines


def test_host_layer_writes_the_reference_gene_file(kgx, tmp_path):
    """GpuGeneGenotypes (csrc/host/kga_analysis_gpu_gene.cpp) on a 60-genome population with 20 genes: the CSV it writes, line
    for line, against the restatement with zlib.crc32 keys.  (kgx_genotype_statistics itself is checked against the reference's
    operation order in test_genotype_statistics_cpu.py.)"""
    from tests import host_api as ha

    G, rows_n, n_genes = 60, 300, 20
    rng = np.random.default_rng(60)
    codes = rng.choice(4, size=(rows_n, G), p=[0.8, 0.12, 0.07, 0.01]).astype(np.uint8)
    hgvs = [f"Pf3D7_{1 + r % 14:02d}_v3:g.{1000 + 37 * r}{'ACGT'[r % 4]}>{'CGTA'[r % 4]}" for r in range(rows_n)]
    genes = [rng.choice(rows_n, int(n), replace=False).astype(np.uint32) for n in rng.integers(0, 25, n_genes)]
    genes[3] = np.zeros(0, dtype=np.uint32)
    codes[genes[5]] = 0                                     # a gene nobody carries (rows shared with others go quiet too)
    ids = [f"PF3D7_{100 * i:07d}" for i in range(n_genes)]
    coding_length = np.array([0 if i == 7 else 300 + 91 * i for i in range(n_genes)], dtype=np.uint64)
    detail = [f"gene {i}; erythrocyte membrane protein 1, PfEMP1" for i in range(n_genes)]
    members, first, n_rows = row_lists(genes)
    packed = kgx.pack_dosage2(codes)
    path = tmp_path / "gene_variants.csv"

    def strings(items):
        return (C.c_char_p * len(items))(*[s.encode() for s in items])

    fn = ha.lib().kgxh_gene_genotypes_write
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_void_p, C.POINTER(C.c_char_p),
                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
    error = C.create_string_buffer(512)
    rc = fn(G, rows_n, strings(hgvs), kgx.ptr(packed), None, n_genes, strings(ids), kgx.ptr(coding_length), strings(detail), kgx.ptr(members), kgx.ptr(first),
            kgx.ptr(n_rows), str(path).encode(), error, 512)
    assert rc == 0, error.value.decode()
    got = path.read_text().split("\n")
    assert got[-1] == "" and got[:-1] == python_gene_csv(kgx, codes, hgvs, genes, ids, coding_length, detail)
