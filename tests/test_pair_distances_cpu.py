"""kgx_pair_distances (host only) against its own formulas, bit for bit, and against a per-cell loop in long double.

G = 9 genomes x 50 rows; the counts are the plain product the device test compares kgx_pair_counts with.  Genome 7 is never
called (code 3 everywhere): N = 0 for every pair with it."""
import numpy as np
import pytest

from kgl_gene_amd import capi

G, N_ROWS = 9, 50
CODES = np.random.default_rng(99).choice(4, size=(N_ROWS, G), p=[0.5, 0.25, 0.15, 0.1]).astype(np.uint8)
CODES[:, 7] = 3
Z = np.stack([CODES == 1, CODES == 2, CODES == 3]).astype(np.int64)
FULL = np.einsum("pra,qrb->abpq", Z, Z)                                        # [a][b][kind of a][kind of b]
COUNTS = FULL[np.triu_indices(G)].reshape(-1, 9).astype(np.uint32)
PAIRS = [(a, b) for a in range(G) for b in range(a, G)]
H, M, O = 0, 1, 2


def by_formula(a, b, kind):
    n, own_a, own_b = FULL[a, b], np.diag(FULL[a, a]), np.diag(FULL[b, b])
    called = N_ROWS - own_a[O] - own_b[O] + n[O, O]
    x_a = (own_a[H] - n[H, O]) + 2 * (own_a[M] - n[M, O])
    x_b = (own_b[H] - n[O, H]) + 2 * (own_b[M] - n[O, M])
    shared = 2 * (n[H, H] + n[H, M] + n[M, H] + 2 * n[M, M]) if kind == 0 else n[H, H] + 2 * n[H, M] + 2 * n[M, H] + 4 * n[M, M]
    return np.float64(np.nan) if called == 0 else np.float64(int(x_a + x_b - shared)) / np.float64(int(2 * called))


def by_cells(a, b, kind):
    both = (CODES[:, a] != 3) & (CODES[:, b] != 3)
    x_a, x_b = CODES[both, a].astype(np.longdouble), CODES[both, b].astype(np.longdouble)
    f_a, f_b = x_a / 2, x_b / 2
    cells = np.abs(x_a - x_b) / 2 if kind == 0 else f_a * (1 - f_b) + f_b * (1 - f_a)
    return cells.sum() / np.longdouble(both.sum()) if both.any() else np.longdouble(np.nan)


@pytest.mark.parametrize("kind", [0, 1])
def test_distances(kind):
    got = capi.pair_distances(COUNTS, G, N_ROWS, kind)
    for (a, b), value in zip(PAIRS, got):
        assert capi.pair_index(a, b, G) == PAIRS.index((a, b))
        want, cells = by_formula(a, b, kind), by_cells(a, b, kind)
        if 7 in (a, b):
            assert np.isnan(value) and np.isnan(want) and np.isnan(cells)
            continue
        assert value.tobytes() == want.tobytes(), (a, b, value, want)
        assert abs(np.longdouble(value) - cells) <= np.spacing(value), (a, b, value, cells)
    assert np.nanmax(got) > 0.0
    if kind == 0:
        assert got[capi.pair_index(0, 0, G)] == 0.0            # a genome is identical by state to itself


def test_a_bad_kind_is_refused():
    out = np.zeros(len(PAIRS))
    assert capi.lib().kgx_pair_distances(capi.ptr(COUNTS), G, N_ROWS, 2, capi.ptr(out)) == capi.KGX_EINVAL
    assert "kind" in capi.lib().kgx_last_error().decode()
    assert capi.lib().kgx_pair_distances(capi.ptr(COUNTS), G, N_ROWS, 0, None) == capi.KGX_EINVAL
