"""kgx_ld_statistics (host only) against exact integers: cov, vx, vy as Python integers from the cells themselves, and
cov / sqrt(vx vy) in long double.  The tables are the plain product the device test compares kgx_ld_counts with.

The library's value is three integer-to-double conversions, one multiplication, one square root and one division: at most
4.5 x 2^-53 ~ 5e-16 from the exact quotient; the tolerance is that bound with a 20-fold margin."""
import math

import numpy as np

from kgl_gene_amd import capi

G, N_ROWS, WINDOW = 50, 14, 15                                                 # a window past the list: every pair, and entries past the end
RTOL = 1e-14
CODES = np.random.default_rng(123).choice(4, size=(N_ROWS, G), p=[0.45, 0.25, 0.2, 0.1]).astype(np.uint8)
CODES[3] = 1                                                                   # a constant row
CODES[4] = 3                                                                   # never called
CODES[5, : G // 2], CODES[6, G // 2 :] = 3, 3                                  # rows 5 and 6 are never called together: N == 0
CODES[8] = np.array([2, 1, 0, 3], dtype=np.uint8)[CODES[7]]                    # row 7's complement-coded twin (0 <-> 2)
Z = np.stack([CODES == 1, CODES == 2, CODES == 3]).astype(np.int64)
FULL = np.einsum("pig,qjg->ijpq", Z, Z).reshape(N_ROWS, N_ROWS, 9)
COUNTS = np.zeros((N_ROWS, WINDOW + 1, 9), dtype=np.uint32)
for _i in range(N_ROWS):
    COUNTS[_i, : N_ROWS - _i] = FULL[_i, _i:]
R = capi.ld_statistics(COUNTS, G)


def exact(i, j):
    """(N, cov, vx, vy) over the genomes both rows are called in, as Python integers"""
    both = (CODES[i] != 3) & (CODES[j] != 3)
    x, y = [int(v) for v in CODES[i][both]], [int(v) for v in CODES[j][both]]
    N, Sx, Sy = len(x), sum(x), sum(y)
    return (N, N * sum(a * b for a, b in zip(x, y)) - Sx * Sy, N * sum(a * a for a in x) - Sx * Sx, N * sum(b * b for b in y) - Sy * Sy)


def test_every_entry():
    assert R.shape == (N_ROWS, WINDOW + 1) and R.dtype == np.float64
    defined = 0
    for i in range(N_ROWS):
        for d in range(WINDOW + 1):
            if i + d >= N_ROWS:
                assert math.isnan(R[i, d])                     # past the list's end
                continue
            N, cov, vx, vy = exact(i, i + d)
            if N == 0 or vx == 0 or vy == 0:
                assert math.isnan(R[i, d]), (i, d)
                continue
            want = np.longdouble(cov) / np.sqrt(np.longdouble(vx) * np.longdouble(vy))
            assert abs(np.longdouble(R[i, d]) - want) <= RTOL * abs(want), (i, d, R[i, d], want)
            defined += 1
    assert defined > 40


def test_undefined_and_fixed_values():
    assert np.isnan(R[3, : N_ROWS - 3]).all() and np.isnan([R[i, 3 - i] for i in range(4)]).all()                    # the constant row
    assert np.isnan(R[4, : N_ROWS - 4]).all() and np.isnan([R[i, 4 - i] for i in range(5)]).all()                    # the all-O row
    assert exact(5, 6)[0] == 0 and math.isnan(R[5, 1])                                                               # N == 0
    for i in range(N_ROWS):
        assert R[i, 0] == 1.0 or exact(i, i)[2] == 0           # a row against itself: exactly 1
    assert exact(7, 7)[2] > 0 and R[7, 1] == -1.0              # ... and against its complement-coded twin: exactly -1
