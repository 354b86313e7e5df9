"""kgx_ibd_tables / kgx_ibd_carry (host only) against the formulas of include/kgx.h in np.longdouble.

The identity: g(0) + g(1) = 1 and sum_x P(x | z) = 1, so each state's table sums to 1 over the four ORDERED allele pairs --
e[0] + 2 e[2] + e[5] = 1, the off-diagonal class (0, 1) standing for (0, 1) and (1, 0)."""
import numpy as np
import pytest

from kgl_gene_amd import capi

LD, EPS = np.longdouble, 1e-3


COUNTS = np.random.default_rng(11).integers(1, 5000, size=(40, 4)).astype(np.uint32)
COUNTS[:4] = (0, 5, 0, 9), (7, 5, 0, 9), (0, 5, 7, 9), (1, 0, 4_000_000_000, 0)                  # nothing called; p = 0; p = 1; p near 1


def test_tables_are_the_formulas_rounded_once():
    c, got = COUNTS, capi.ibd_tables(COUNTS, EPS)
    p1 = c[:, 2].astype(LD) / (c[:, 0].astype(LD) + c[:, 2].astype(LD)).clip(1)
    p, eps = np.stack([1 - p1, p1]), LD(EPS)                                      # (double)EPS exactly, as the library gets it
    g = p * (1 - eps) + (1 - p) * eps
    hit = np.where(np.eye(2, dtype=bool), 1 - eps, eps)                           # P(x | z)
    want = np.ones((len(c), 2, 6), dtype=LD)
    for k, (x, y) in {0: (0, 0), 2: (0, 1), 5: (1, 1)}.items():
        want[:, 0, k] = g[x] * g[y]
        want[:, 1, k] = sum(p[z] * hit[x, z] * hit[y, z] for z in range(2))
    want[:3] = 1                                                                  # the degenerate rows say nothing
    assert got.dtype == np.float32 and (got[:3] == 1).all() and (got[:, :, [1, 3, 4]] == 1).all() and (got[3:, :, [0, 2, 5]] != 1).all()
    assert (np.abs(got.astype(LD) - want) <= np.spacing(got).astype(LD) * LD(0.5000001)).all()       # one rounding of a double result
    total = got[3:, :, 0].astype(LD) + 2 * got[3:, :, 2].astype(LD) + got[3:, :, 5].astype(LD)
    assert (np.abs(total - 1) <= LD(2) ** -23 * LD(1.001)).all()                  # entries below 1, each within half a float ulp (2^-25), four of them


def test_carry_is_one_exp():
    position = np.cumsum(np.random.default_rng(12).integers(0, 50_000, size=300)).astype(np.uint32)
    start = np.zeros(300, dtype=np.uint8)
    start[[100, 101]] = 1
    position[100:] -= position[100]                                               # positions start again: not without the contig start
    got = capi.ibd_carry(position, 1e-5, start)
    step = np.diff(position.astype(np.int64), prepend=0).astype(LD)
    want = np.exp(-(np.float64(1e-5) * step.astype(np.float64)).astype(LD))       # the product is the library's one double multiplication
    assert (got[[0, 100, 101]] == 0).all() and got[1:100].min() > 0
    called = got > 0
    assert (np.abs(got.astype(LD) - want)[called] <= np.spacing(got[called])).all()
    assert (capi.ibd_carry(position[:100], 0.0) == np.r_[0.0, np.ones(99)]).all()


def test_refusals():
    position = np.array([10, 20, 5], dtype=np.uint32)
    with pytest.raises(capi.KgxError, match=r"position\[2\]") as refused:
        capi.ibd_carry(position, 1e-5)
    assert refused.value.code == capi.KGX_EINVAL
    for rate in (-1.0, np.nan, np.inf):
        with pytest.raises(capi.KgxError, match="rate"):
            capi.ibd_carry(position[:2], rate)
    for eps in (0.0, 0.6, np.nan):
        with pytest.raises(capi.KgxError, match="eps"):
            capi.ibd_tables(COUNTS, eps)
    assert capi.lib().kgx_ibd_tables(None, 3, EPS, None) == capi.KGX_EINVAL and capi.lib().kgx_ibd_carry(None, None, 3, 1e-5, None) == capi.KGX_EINVAL
