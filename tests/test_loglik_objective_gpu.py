"""logLikelihood(F) as the device computes it -- kgx_inbreed_objective by one pass over the bytes (every flavour the plan
can choose for mode 2) and by the per-genome moments with the exact walk next to the floor -- against the plain
long-double statement of the same sum (tests/loglik_reference.py, pinned to the oracle without a GPU in
tests/test_loglik_reference_cpu.py): the VALUE, per genome, at points on the kinks, next to both bounds and across the
box, not the maximiser alone.  Then the search's result rated by the reference's objective, and HallME's 50 steps
against the same cells.  Tolerances: 1e-9 * sum|log p| for an evaluation and 1e-9 for HallME -- the bounds the project
already holds its paths to, ceilings, not measurements; what was measured is printed.  Needs a GPU."""
import functools

import numpy as np
import pytest

from . import loglik_populations as lp
from . import loglik_reference as lr
from . import oracle_api as oa

pytestmark = pytest.mark.gpu

REL = 1e-9
HALL = 1e-9
START_SEED = 77
COUNT_FIELDS = ["major_hetero_count", "minor_hetero_count", "minor_homo_count", "major_homo_count", "total_allele_count"]
FLAVOURS = {"table pass": {}, "four genomes a lane": {"KGX_K5_EVAL_GPL": "4"}, "generic": {"KGX_K5_GENERIC": "1"},
            "no tables": {"KGX_K5_NO_EVAL_LUT": "1"}}
POPULATIONS = ["S1 phased ALL", "S1 phased 2", "S1 unphased ALL", "S1 unphased 2", "S2", "S2 indexed", "S3"]


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything about one population that does not need the device: the matrix's bytes, the table and the selection a
    call is given, and the reference's values at the point sets (P1..P10) -- computed once, shared by every test."""
    if name.startswith("S1"):
        _, phase, sp = name.split()
        pop = lp.window_population(oa.Population.PHASED if phase == "phased" else oa.Population.UNPHASED)
        table, sel = pop["windows"][oa.ALL if sp == "ALL" else int(sp)]
        matrix, index, table, phased = pop["rows"], sel, np.ascontiguousarray(table[sel]), pop["phased"]
    elif name.startswith("S2"):
        pop = lp.synth_population()
        matrix, index, table, phased = pop["rows"], None, pop["table"], True
        if name == "S2 indexed":
            index = np.sort(np.random.default_rng(41).choice(lp.SYNTH_L, 4501, replace=False)).astype(np.uint32)
            table = np.ascontiguousarray(table[index])
    else:
        pop = lp.edge_population()
        matrix, index, table, phased = pop["rows"], None, pop["table"], True
        if name == "S3 quiet":
            index = pop["quiet"]
            table = np.ascontiguousarray(table[index])
    rows = matrix if index is None else matrix[index]
    cells = lr.classify(rows, table, phased)
    points = lr.point_sets(rows.shape[1], lr.median_kink(rows, table, phased, cells=cells))
    want = {p: lr.loglikelihood(rows, table, phased, F, cells=cells) for p, F in points.items()}
    served = {p: lr.served_by_moments(rows, table, phased, F, cells=cells) for p, F in points.items()} if phased else None
    return dict(name=name, matrix=matrix, index=index, table=table, phased=phased, rows=rows, cells=cells, points=points, want=want, served=served,
                G=rows.shape[1], synthetic=name.startswith("S2"))


def device_matrix(kgx, c):
    m = kgx.GenotypeMatrix(c["G"], c["matrix"].shape[0])
    if c["synthetic"]:
        m.synth_multiallelic(1111, 0, 0)
    else:
        m.load_rows(c["matrix"])
    assert np.array_equal(m.read_rows(), c["matrix"])
    return m


def relative_error(got, want, magnitude):
    return np.abs(got.astype(np.longdouble) - want) / magnitude


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("population", POPULATIONS)
def test_objective_by_passes_is_the_reference(kgx, monkeypatch, population, flavour):
    """One pass over the bytes -- the table pass with eight and with four genomes a lane (k_inbreed_eval_lut<2>), the generic
    kernel (k_inbreed_sweep<2>) under both switches that lead to it -- at every point set, over all genomes and over a
    range off the lanes' width: every value finite and within the bound of the reference's."""
    for key, value in FLAVOURS[flavour].items():
        monkeypatch.setenv(key, value)
    c = case(population)
    m = device_matrix(kgx, c)
    G = c["G"]
    worst = 0.0
    for g0, g1 in ((0, G), (8, G - 3)):
        for p, F in c["points"].items():
            want, magnitude = c["want"][p]
            got = m.inbreed_objective(c["table"], F[g0:g1], phased=c["phased"], locus_index=c["index"], g0=g0, g1=g1, by_passes=True)
            assert np.isfinite(got).all(), (population, flavour, p, g0, g1)
            rel = relative_error(got, want[g0:g1], magnitude[g0:g1])
            worst = max(worst, float(rel.max()))
            assert rel.max() <= REL, (population, flavour, p, g0, g1, float(rel.max()), g0 + int(rel.argmax()), float(F[g0 + int(rel.argmax())]))
    print(f"loglik-objective: {population} | passes | {flavour}: worst |device - reference| / sum|log p| = {worst:.3g}")
    m.close()


@pytest.mark.parametrize("population", ["S1 phased ALL", "S1 phased 2", "S2", "S2 indexed", "S3", "S3 quiet"])
def test_objective_by_moments_is_the_reference(kgx, population):
    """A NaN only for a genome the contract hands to the passes (loglik_reference.served_by_moments states the rule of
    k_loglik_search from the reference's side), a finite value -- within the bound -- for every other."""
    c = case(population)
    G = c["G"]
    # the cap, from the reference alone, before the device is asked: the contract serves almost every (genome, point) outside P8
    if not population.startswith("S3"):
        pairs = np.concatenate([c["served"][p] for p in c["points"] if p != "P8"])
        assert pairs.mean() >= 0.95, (population, float(pairs.mean()))
    named = lp.edge_population()["named"]
    m = device_matrix(kgx, c)
    worst = 0.0
    for p, F in c["points"].items():
        want, magnitude = c["want"][p]
        served = c["served"][p]
        got = m.inbreed_objective(c["table"], F, phased=True, locus_index=c["index"])
        handed = np.isnan(got)
        assert not (handed & served).any(), (population, p, "NaN for a genome the contract serves", np.flatnonzero(handed & served).tolist())
        assert not (~handed & ~served).any(), (population, p, "a value for a genome the contract hands over", np.flatnonzero(~handed & ~served).tolist())
        assert np.isfinite(got[~handed]).all(), (population, p)
        if population.startswith("S3"):
            assert handed[named].all(), (population, p)
        if population == "S3 quiet":
            others = np.setdiff1d(np.flatnonzero(F <= 0.9), named)
            assert not handed[others].any(), (population, p, others[handed[others]].tolist())
        rel = relative_error(got[~handed], want[~handed], magnitude[~handed])
        if rel.size:
            worst = max(worst, float(rel.max()))
            assert rel.max() <= REL, (population, p, float(rel.max()), int(np.flatnonzero(~handed)[rel.argmax()]), float(F[np.flatnonzero(~handed)[rel.argmax()]]))
    print(f"loglik-objective: {population} | moments: worst |device - reference| / sum|log p| = {worst:.3g}")
    m.close()


@pytest.mark.parametrize("population,env,paths", [("S2", {}, ("loglik moments", "loglik moments + passes")),
                                                  ("S3", {}, ("one launch",)),
                                                  ("S3", {"KGX_K7_NO_WAVE": "1"}, ("loglik moments + passes",))])
def test_search_ends_on_a_maximum_of_the_reference_objective(kgx, monkeypatch, population, env, paths):
    """The search itself: the reference's objective at the device's maximiser is not below its objective 2e-6 to either
    side (each side of a search stops at a simplex of 1e-6), up to 1e-9 of its magnitude -- a local maximum of the true
    objective, not of the device's own."""
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    c = case(population)
    m = device_matrix(kgx, c)
    start = kgx.reference_starts("Loglikelihood", START_SEED, c["G"])
    got = m.inbreed(c["table"], "Loglikelihood", phased=True, locus_index=c["index"], start=start)
    assert kgx.inbreed_last_path() in paths, kgx.inbreed_last_path()
    assert np.array_equal(np.stack([got[name] for name in COUNT_FIELDS], axis=1), lr.class_counts(c["cells"][0]))
    at = got["inbred_allele_sum"].copy()
    assert np.isfinite(at).all() and np.all(np.abs(at) <= 1.0)
    value, magnitude = lr.loglikelihood(c["rows"], c["table"], True, at, cells=c["cells"])
    deficit = np.longdouble(0)
    for step in (-2e-6, 2e-6):
        beside, _ = lr.loglikelihood(c["rows"], c["table"], True, np.clip(at + step, -1.0, 1.0), cells=c["cells"])
        short = (beside - value) / magnitude
        deficit = max(deficit, short.max())
        assert np.all(value >= beside - REL * magnitude), (population, step, float(short.max()), int(short.argmax()), float(at[short.argmax()]))
    print(f"loglik-objective: {population} | search on {kgx.inbreed_last_path()}: the reference's objective 2e-6 beside the maximiser exceeds it by "
          f"{float(deficit):.3g} of its magnitude at most")
    m.close()


@pytest.mark.parametrize("population,path,env", [("S3", "one launch", {}),
                                                 ("S3", "hall moments", {"KGX_K7_NO_WAVE": "1"}),
                                                 ("S3", "hall passes", {"KGX_K7_NO_WAVE": "1", "KGX_K7_HALL_PASSES": "1"}),
                                                 ("S2", "hall moments", {"KGX_K7_NO_WAVE": "1"}),
                                                 ("S2", "hall passes", {"KGX_K7_NO_WAVE": "1", "KGX_K7_HALL_PASSES": "1"})])
def test_hallme_is_the_reference(kgx, monkeypatch, population, path, env):
    """HallME's 50 expectation steps -- the same sum over the same cells -- on every path, from the reference's start
    points: within 1e-9 (the project's tolerance against the oracle), the class counts bit for bit."""
    for key, value in env.items():
        monkeypatch.setenv(key, value)
    c = case(population)
    m = device_matrix(kgx, c)
    start = kgx.reference_starts("HallME", START_SEED, c["G"])
    got = m.inbreed(c["table"], "HallME", phased=True, locus_index=c["index"], start=start)
    assert kgx.inbreed_last_path() == path, kgx.inbreed_last_path()
    assert np.array_equal(np.stack([got[name] for name in COUNT_FIELDS], axis=1), lr.class_counts(c["cells"][0]))
    want = hall_reference(population)
    err = np.abs(got["inbred_allele_sum"].astype(np.longdouble) - want)
    assert np.isfinite(got["inbred_allele_sum"]).all() and float(np.abs(want).max()) > 0.05
    print(f"loglik-objective: {population} | HallME on {path}: worst |device - reference| = {float(err.max()):.3g}")
    assert err.max() <= HALL, (population, path, float(err.max()), int(err.argmax()))
    m.close()


@functools.lru_cache(maxsize=None)
def hall_reference(population):
    from kgl_gene_amd import capi

    c = case(population)
    return lr.hall_me(c["rows"], c["table"], True, capi.reference_starts("HallME", START_SEED, c["G"]), cells=c["cells"])
