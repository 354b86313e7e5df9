"""GPU_INBREED with FrequencySource=Population: the allele frequencies come from the diploid population's own AC / AN per super
population (kgx_gt8_allele_census + kgx_census_allele_frequencies) instead of the reference file's INFO fields.

Run A reads a reference file whose frequencies are all 0.25 and replaces them on the device; run B reads, with the default source,
a reference file whose frequencies were set HERE to the restatement's float32(AC / AN) per super population and for ALL.  Both
runs then sample, sweep and write from the same numbers: their result files must be byte-identical.

The reference file is a Gnomad 3.1 mono-genome file: its six super-population fields are distinct (AF_afr, AF_amr, AF_eas, AF_nfe,
AF_sas, AF; kgl_variant_db_freq.h:84-96), and -- unlike a Genome1000 file, which the package takes for the diploid population -- it
is a frequency source.  The diploid population is a phased Genome1000 file with a PED record for most genomes.
"""
import copy
from functools import lru_cache

import numpy as np
import pytest

from . import allele_census_reference as acr
from . import inbreed_inputs as ii
from . import oracle_api as oa
from . import records_io as rio
from . import synth_vcf as sv

pytestmark = pytest.mark.gpu

G, L = 62, 1500
POPS = ["AFR", "AMR", "EAS", "EUR", "SAS"]
GNOMAD3_FIELDS = ["AF_afr", "AF_amr", "AF_eas", "AF_nfe", "AF_sas", "AF"]
PARAMS = dict(AnalysisType="false", OutputFile="inbreed", MinAlleleFreq=0.02, MaxAlleleFreq=0.9, LowerWindow=0, UpperWindow=60000, LociiCount=150,
              SamplingDistance=40, StartPoints="Midpoint")


@lru_cache(maxsize=None)
def case():
    """(records with every AF 0.25, records with the population's own AFs, gt, ids, ped, the AF table [n_loci][amax][6])."""
    rec, gt = sv.multiallelic_block(G, L, rng_seed=77)
    ids = sv.genome_ids(G, prefix="NA")
    ped = [(g, POPS[(i * 7) % 5]) for i, g in enumerate(ids) if i not in (13, 40)]     # two genomes have no PED record: on no device column
    flat = copy.deepcopy(rec)
    flat.af = [np.full_like(np.asarray(a, dtype=np.float32).reshape(-1, 6), 0.25) for a in rec.af]

    loci = ii.ReferenceLoci(rec)
    cells = ii.encode_gt8(rec, gt, loci, phased_order=True)                            # [n_loci][G], what the package uploads
    ped_map = dict(ped)
    groups = np.array([oa.SUPER_POPS.index(ped_map[g]) if g in ped_map else 0xFF for g in ids], dtype=np.uint8)
    amax = max(len(a) for a in loci.alts)
    n_alt = np.array([len(a) for a in loci.alts], dtype=np.uint8)
    words = acr.census(cells, groups, 6, amax)
    sizes = acr.group_sizes(groups, 6)
    table = np.stack([acr.allele_frequencies(words, sizes, list(range(6)) if sp == oa.ALL else [sp], n_alt) for sp in range(6)], axis=-1)
    assert sizes[:5].min() >= 10 and sizes[5] == 0 and not np.isnan(table[:, 0, :]).any()

    # the same alts in the same order as ReferenceLoci lists them: (record, alt) of every (locus, place)
    own = copy.deepcopy(rec)
    own.af = [np.array(a, dtype=np.float32).reshape(-1, 6).copy() for a in rec.af]
    place = {}
    index_of = {int(o): l for l, o in enumerate(loci.offsets)}
    for r in range(rec.n_records):
        for a, alt in enumerate(rec.alts[r]):
            if not ii.is_snp(rec.refs[r], alt):
                continue
            l = index_of[int(rec.offsets[r])]
            j = place.get(l, 0)
            place[l] = j + 1
            assert loci.alts[l][j] == (rec.refs[r], alt)
            own.af[r][a, :] = table[l, j, :].astype(np.float32)
    return flat, own, gt, ids, ped, table


def run(tmp_path, monkeypatch, name, reference, algorithm, **extra):
    flat, own, gt, ids, ped, _ = case()
    work = tmp_path / name
    work.mkdir()
    monkeypatch.setitem(rio.AF_FIELDS, "Gnomad3_1", GNOMAD3_FIELDS)
    ref_path, dip_path = work / "gnomad.bin", work / "diploid.bin"
    rio.write_records(ref_path, reference, None, ["Reference"], oa.Population.REFERENCE, "Gnomad3_1", population_id="Gnomad")
    rio.write_records(dip_path, flat, gt, ids, oa.Population.PHASED, "Genome1000", population_id="Diploid", ped=ped)
    res = rio.run_driver("GPU_INBREED", work, [ref_path, dip_path], Algorithm=algorithm, **PARAMS, **extra)
    assert res.returncode == 0, res.stderr
    return (work / "inbreed.csv").read_bytes(), (work / "inbreed_detail.csv").read_bytes()


@pytest.mark.parametrize("algorithm", ["Simple", "RitlandLocus", "HallME", "Loglikelihood"])
def test_population_source_equals_a_reference_file_of_the_same_frequencies(tmp_path, monkeypatch, kgx, algorithm):
    flat, own, _, ids, ped, _ = case()
    from_population = run(tmp_path, monkeypatch, "a", flat, algorithm, FrequencySource="Population")
    from_file = run(tmp_path, monkeypatch, "b", own, algorithm)
    assert from_population[0] == from_file[0]
    assert from_population[1] == from_file[1]
    header, rows = rio.read_csv(tmp_path / "a" / "inbreed_detail.csv")
    assert len({r[0] for r in rows}) >= 2 and len({r[1] for r in rows}) == len(ped)      # several windows, every genome with a PED record
    assert any(int(r[10]) > 0 for r in rows)


def test_population_source_is_not_ignored(tmp_path, monkeypatch, kgx):
    flat = case()[0]
    from_population = run(tmp_path, monkeypatch, "a", flat, "Simple", FrequencySource="Population")
    spelled_out = run(tmp_path, monkeypatch, "r", flat, "Simple", FrequencySource="Reference")
    default = run(tmp_path, monkeypatch, "d", flat, "Simple")
    assert spelled_out == default                                  # "Reference" is today's behaviour
    assert from_population[1] != default[1]


def test_unknown_frequency_source_disables_the_package(tmp_path, monkeypatch, kgx):
    flat, _, gt, ids, ped, _ = case()
    monkeypatch.setitem(rio.AF_FIELDS, "Gnomad3_1", GNOMAD3_FIELDS)
    ref_path, dip_path = tmp_path / "gnomad.bin", tmp_path / "diploid.bin"
    rio.write_records(ref_path, flat, None, ["Reference"], oa.Population.REFERENCE, "Gnomad3_1", population_id="Gnomad")
    rio.write_records(dip_path, flat, gt, ids, oa.Population.PHASED, "Genome1000", population_id="Diploid", ped=ped)
    res = rio.run_driver("GPU_INBREED", tmp_path, [ref_path, dip_path], Algorithm="Simple", **PARAMS, FrequencySource="Cohort")
    assert res.returncode == 1 and "initializeAnalysis failed" in res.stderr
