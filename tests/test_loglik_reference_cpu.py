"""tests/loglik_reference.py -- the numpy statement of logLikelihood(F) the device is measured against
(tests/test_loglik_objective_gpu.py) -- pinned to the oracle, which stays the statement of the reference's semantics:
the objective of every genome at every point set, and the class counts, on the window population and on the C5-style
synthetic one; then a handful of cells worked by hand.  No GPU.

The tolerance is derived, not measured.  Both sides compute each cell's probability in the same double operations
(the oracle is built with -ffp-contract=off; numpy does not contract), so the terms differ by one rounding of each log
(the oracle's, in double; numpy's are long double), and the oracle adds its N terms one by one in double:
|oracle - reference| <= (N + 2) * 2^-52 * sum|log p| per genome -- recursive summation, (N - 1) * 2^-53 to first
order, plus the logs' roundings, with room for the second order."""
import numpy as np
import pytest

from . import loglik_populations as lp
from . import loglik_reference as lr
from . import oracle_api as oa

EPS = 2.0 ** -52


def _check_against_oracle(name, rows, table, phased, oracle_at):
    cells = lr.classify(rows, table, phased)
    n_cells = lr.class_counts(cells[0])[:, 4].astype(np.float64)
    worst = 0.0
    for point_set, F in lr.point_sets(rows.shape[1], lr.median_kink(rows, table, phased, cells=cells)).items():
        want = oracle_at(F)
        got, magnitude = lr.loglikelihood(rows, table, phased, F, cells=cells)
        assert np.isfinite(want).all() and np.isfinite(got).all(), (name, point_set)
        err = np.abs(want.astype(np.longdouble) - got)
        bound = (n_cells + 2.0) * EPS * magnitude
        worst = max(worst, float((err / magnitude).max()))
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, (name, point_set, bad.tolist()[:5], [float(x) for x in err[bad][:5]], [float(x) for x in bound[bad][:5]])
    print(f"{name}: oracle against the numpy reference, worst |difference| / sum|log p| = {worst:.3g}")


@pytest.mark.parametrize("mode", [oa.Population.PHASED, oa.Population.UNPHASED])
def test_reference_is_the_oracle_on_the_window_population(mode):
    pop = lp.window_population(mode)
    for sp, (table, sel) in pop["windows"].items():
        rows = np.ascontiguousarray(pop["rows"][sel][:, pop["order"]])          # the oracle's genome order
        assert len(sel) > 300
        counts = lr.class_counts(lr.classify(rows, table[sel], pop["phased"])[0])
        assert np.array_equal(counts, lp.oracle_counts(pop, sp)), sp
        assert counts[:, 1].sum() > 0 and counts[:, 2].sum() + counts[:, 1].sum() > 0 and (counts[:, 4] < len(sel)).any()
        _check_against_oracle(f"window population, mode {mode}, super population {sp}", rows, table[sel], pop["phased"],
                              lambda F: lp.oracle_objective(pop, sp, F))


def test_reference_is_the_oracle_on_the_synthetic_population():
    pop = lp.synth_population()
    rows = np.ascontiguousarray(pop["rows"][:, pop["order"]])
    counts = lr.class_counts(lr.classify(rows, pop["table"], True)[0])
    assert np.array_equal(counts, lp.synth_oracle_counts(pop))
    assert counts[:, :4].min() > 0
    _check_against_oracle("synthetic population", rows, pop["table"], True, lambda F: lp.synth_oracle_objective(pop, F))


def test_hand_worked_cells():
    """One locus a class, binary-exact values: the classifier, the objective, the helpers and a HallME step by hand."""
    nan = np.nan
    table = np.array([
        [0.25, 0.125],      # 0 p_major 0.625
        [0.25, 0.125],      # 1
        [0.25, 0.125],      # 2
        [0.25, 0.125],      # 3
        [0.25, 0.125],      # 4
        [0.25, nan],        # 5 an alt without a frequency
        [0.5, 0.5],         # 6 p_major 0: no major homozygote
        [0.75, 0.5],        # 7 sum 1.25: not valid
        [nan, nan],         # 8 no frequency: not valid
        [0.75, 0.25],       # 9 p_major 0 <= 0.01
        [1.5, -3.0],        # 10 clipped to 1 and 0: valid, p_major 0
    ])
    rows = np.array([[0x00], [0x01], [0x11], [0x21], [0x10], [0x02], [0x00], [0x01], [0x00], [0x11], [0x12]], dtype=np.uint8)
    rows = np.concatenate([rows, np.array([[0x0F], [0xFF], [0x03], [0x31], [0x20], [0x21], [0x21], [0x11], [0x01], [0x00], [0x22]], dtype=np.uint8)], axis=1)
    cls, f1, f2 = lr.classify(rows, table, phased=True)
    assert cls[:, 0].tolist() == [lr.MAJOR_HOM, lr.MAJOR_HET, lr.MINOR_HOM, lr.MINOR_HET, lr.MINOR_HET, lr.NONE, lr.NONE, lr.NONE, lr.NONE,
                                  lr.MINOR_HOM, lr.MINOR_HET]
    assert np.nan_to_num(f1[:, 0]).tolist() == [0.625, 0.25, 0.25, 0.25, 0.25, 0, 0, 0, 0, 0.75, 0.0]
    assert np.nan_to_num(f2[:, 0]).tolist() == [0.625, 0.625, 0.25, 0.125, 0.25, 0, 0, 0, 0, 0.75, 1.0]
    # the second genome: 15, 0xFF, indices past amax, (0, 2), a pair with a missing frequency, the pair at p_major 0, nothing where
    # the locus is not valid, a homozygote of an alt clipped to 0
    assert cls[:, 1].tolist() == [lr.NONE, lr.NONE, lr.NONE, lr.NONE, lr.MINOR_HET, lr.NONE, lr.MINOR_HET, lr.NONE, lr.NONE, lr.NONE, lr.MINOR_HOM]
    assert (f1[4, 1], f2[4, 1]) == (0.125, 0.125) and (f1[6, 1], f2[6, 1]) == (0.5, 0.5) and (f1[10, 1], f2[10, 1]) == (0.0, 0.0)
    # an unphased population: (a, a) is a heterozygote of that allele twice
    cls_u, f1_u, f2_u = lr.classify(rows, table, phased=False)
    assert cls_u[2, 0] == lr.MINOR_HET and (f1_u[2, 0], f2_u[2, 0]) == (0.25, 0.25)
    assert np.array_equal(cls_u[[0, 1, 3, 4]], cls[[0, 1, 3, 4]])
    assert lr.class_counts(cls).tolist() == [[1, 3, 2, 1, 7], [0, 2, 1, 0, 3]]

    # the objective at F = 0.5 (every product exact) and at F = -1 (the homozygote of 0.25 under the floor, the pair past 1)
    ln = lambda x: np.log(np.longdouble(x))
    value, magnitude = lr.loglikelihood(rows, table, True, np.array([0.5, 0.5]))
    # major hom 0.5*0.625 + 0.5*0.625^2; major het 2*0.5*0.25*0.625; minor hom 0.5*0.25 + 0.5*0.0625; (1, 2) 2*0.5*0.25*0.125;
    # (0, 1) 2*0.5*0.25*0.25; locus 9: 0.5*0.75 + 0.5*0.5625; locus 10: 2*0.5*0*1 -> the floor
    want0 = ln(0.5078125) + ln(0.15625) + ln(0.15625) + ln(0.03125) + ln(0.0625) + ln(0.65625) + ln(1e-10)
    want1 = ln(0.015625) + ln(0.25) + ln(1e-10)                       # (0, 2); (1, 2) at 0.5, 0.5; y = 0
    assert abs(value[0] - want0) <= 4 * np.finfo(np.longdouble).eps * abs(want0) and abs(value[1] - want1) <= 4 * np.finfo(np.longdouble).eps * abs(want1)
    assert np.array_equal(magnitude, -value)
    value, _ = lr.loglikelihood(rows, table, True, np.array([-1.0, -1.0]))
    # F = -1: major hom -0.625 + 2*0.390625 = 0.15625; major het 4*0.25*0.625 = 0.625; minor hom -0.25 + 0.125 < 0 -> floor;
    # (1, 2) 4*0.25*0.125 = 0.125; (0, 1) 4*0.0625 = 0.25; locus 9 -0.75 + 1.125 = 0.375; locus 10: floor
    want0 = ln(0.15625) + ln(0.625) + ln(1e-10) + ln(0.125) + ln(0.25) + ln(0.375) + ln(1e-10)
    want1 = ln(0.0625) + ln(1.0) + ln(1e-10)                          # (1, 2) at 0.5, 0.5: 4*0.25 = 1, the upper bound
    assert abs(value[0] - want0) <= 4 * np.finfo(np.longdouble).eps * abs(want0) and abs(value[1] - want1) <= 4 * np.finfo(np.longdouble).eps * abs(want1)

    # helpers
    smallest, largest = lr.het_products(rows, table, True)
    assert smallest.tolist() == [0.0, 0.03125] and largest.tolist() == [0.3125, 0.5]
    with_term, _ = lr.het_products(rows, table, True, at_least=lr.TINY_HET, at_most=lr.BIG_HET)
    assert with_term.tolist() == [0.0625, 0.03125]
    k = lr.kinks(rows, table, True)
    assert np.nan_to_num(k[:, 0], nan=9.0).tolist() == [9.0, 9.0, -0.25 / 0.75, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0]      # (0.625, 0.75: kinks past -1)
    assert lr.median_kink(rows, table, True).tolist() == [-0.25 / 0.75, -0.25]
    # every index pair of the table: the smallest product with a term is (0, 2) at 0.125 -- 2 * 0.125^2; clipped 0 and 1 give 0
    assert lr.tabulated_het_floor(table, True) == 0.03125
    served = lr.served_by_moments(rows, table, True, np.array([0.0, 1.0 - 1e-9]))
    assert served.tolist() == [True, False]            # 1e-9 * 0.03125 < 1e-10, and 1e-9 > 2e-10
    assert lr.served_by_moments(rows, table, True, np.array([1.0 - 1e-12, 0.5])).tolist() == [True, True]

    # one HallME step from 0.5: homozygous cells 0.5 / (0.5 + 0.5 * y) over all cells
    one = lr.hall_me(rows, table, True, np.array([0.5, 0.5]), steps=1)
    assert abs(float(one[0]) - (1 / 1.625 + 1 / 1.25 + 1 / 1.75) / 7) < 1e-15 and abs(float(one[1]) - (1.0 / 1.0) / 3) < 1e-15
    assert np.array_equal(lr.hall_me(rows, table, True, one, steps=49), lr.hall_me(rows, table, True, np.array([0.5, 0.5])))


def test_edge_population_is_what_it_says():
    """The constructed population of the GPU tests: its edges are there, and its claims about heterozygous products hold."""
    pop = lp.edge_population()
    rows, table = pop["rows"], pop["table"]
    f, valid, p_major = lr.locus_tables(table)
    cells = lr.classify(rows, table, True)
    cls = cells[0]
    assert not valid[pop["not_valid"]] and valid[pop["barely_valid"]] and p_major[pop["barely_valid"]] == 0.0
    assert (cls[pop["not_valid"]] == lr.NONE).all() and (cls[pop["barely_valid"]] != lr.NONE).any()
    assert (p_major[pop["major_loci"]] > 0.01).tolist() == [False, True, False, True]
    assert p_major[pop["major_loci"][0]] < 0.01 and p_major[pop["major_loci"][1]] - p_major[pop["major_loci"][0]] == 2.0 ** -53
    for locus, has_major in zip(pop["major_loci"], [False, True, False, True]):
        assert ((cls[locus] == lr.MAJOR_HOM).any()) == has_major and (rows[locus] == 0).any() and (cls[locus] == lr.MINOR_HOM).any()
    present = table[~np.isnan(table)]
    assert not ((present > 0.0) & (present < 2.0 ** -20)).any() and (present == 2.0 ** -20).any() and (present == 0.0).any()
    for k in range(1, 21):
        assert (present == 2.0 ** -k).any() and (present == np.nextafter(2.0 ** -k, 1.0)).any()
    # seven classes of homozygous cell, homozygotes at 2^-20, every odd byte
    a1 = rows & 15
    for a in range(1, 7):
        assert ((cls == lr.MINOR_HOM) & (a1 == a)).any(), a
    assert ((cls == lr.MINOR_HOM) & (cells[1] == 2.0 ** -20)).any() and ((cls == lr.MINOR_HOM) & (cells[1] == 0.0)).any()
    assert (cls == lr.MAJOR_HOM).sum(axis=0).min() > 1200
    for byte in (0x07, 0x70, 0x0F, 0xFF):
        assert (rows == byte).any()
    assert ((a1 == 0) & (rows != 0) & (cls == lr.MINOR_HET)).any()
    # heterozygous products: past 1/2 in the named genomes alone; the smallest with a term, tabulated, over the quiet loci
    _, largest = lr.het_products(rows, table, True, cells=cells)
    assert np.array_equal(np.flatnonzero(largest > 0.5), pop["named"])
    assert 5e-11 <= lr.tabulated_het_floor(table, True) < 1.0000001e-9
    quiet = pop["quiet"]
    assert len(quiet) == pop["L"] - 6 and 0.1 * lr.tabulated_het_floor(table[quiet], True) >= lr.FLOOR_MARGIN
    served = lr.served_by_moments(rows[quiet], table[quiet], True, np.full(pop["G"], 0.9))
    assert np.array_equal(np.flatnonzero(~served), pop["named"])
