"""kgx_pair_hmm on the device against a plain scaled forward-backward pass in np.longdouble, row by row and vectorised over the
pairs: a different algorithm (the device runs forward only and carries the IBD weight with the path) on the same inputs.  Every
pair, both fields, within include/kgx.h's bound: with u = 2^-53 and n rows, |d loglik| <= 16 n u + 4 u |loglik| and |d ibd| <=
32 n u ibd (sums of products of non-negative numbers: the relative error grows by the roundings on a path, at most 6 a step for F
and 8 for V, doubled).

1100 rows; random codes plus crafted genomes: 1 a copy of 0; 2 all no-call; 3 a copy of 0 with no-calls over tile edges; 4 all het.
G in {20, 33, 70}: a partial 32-genome tile; a one-genome tail tile; three tiles, so diagonal and off-diagonal tile pairs.  n_rows
around the rescale every 16 positions (15, 16, 17) and the 64-row tile (64, 65), eight tiles and a tail (513), and 1100."""
from functools import lru_cache

import numpy as np
import pytest

from kgl_gene_amd import capi

pytestmark = pytest.mark.gpu

LD = np.longdouble
V, PI, EPS, RATE, U = 1100, 0.3, 1e-3, 1e-4, LD(2) ** -53
CLASS = np.array([[0, 1, 2, 6], [1, 3, 4, 6], [2, 4, 5, 6], [6, 6, 6, 6]])      # include/kgx.h's k of (ca, cb); 6 = neutral


@lru_cache(maxsize=None)
def codes_of(G):
    codes = np.random.default_rng(9000 + G).choice(4, size=(V, G), p=[0.70, 0.03, 0.22, 0.05]).astype(np.uint8)
    codes[:, 1] = codes[:, 0]
    codes[:, 2] = 3
    codes[:, 3] = codes[:, 0]
    codes[[0, *range(60, 70), *range(505, 526), V - 1], 3] = 3
    codes[:, 4] = 1
    return codes


@lru_cache(maxsize=None)
def inputs(G, n_rows, listed, weighted=False, emit_value=None):       # (codes [n][G], rows or None, emit, carry, weight or None)
    rng = np.random.default_rng(n_rows)
    rows = rng.permutation(V)[:n_rows].astype(np.uint32) if listed else None     # shuffled, and one row twice
    if listed:
        rows[-1] = rows[0]
    codes = codes_of(G)[:n_rows] if rows is None else codes_of(G)[rows]
    counts = np.stack([(codes == c).sum(axis=1) for c in range(4)], axis=1)
    emit = capi.ibd_tables(counts, EPS) if emit_value is None else np.full((n_rows, 2, 6), emit_value, dtype=np.float32)
    position = np.cumsum(rng.integers(1, 2000, size=n_rows)).astype(np.uint32)
    start = np.zeros(n_rows, dtype=np.uint8)
    for at in (150, 520, 576):                                                   # further contigs (576: on a tile edge)
        if n_rows > at:
            start[at] = 1
            position[at:] -= position[at] - 5
    return codes, rows, emit, capi.ibd_carry(position, RATE, start), rng.uniform(0.0, 3.0, size=n_rows) if weighted else None


@lru_cache(maxsize=None)
def expected(*key):
    """[G (G + 1) / 2][2] long double: forward and backward passes, each scaled to sum 1 per row."""
    codes, _, emit, carry, weight = inputs(*key)
    n, G = codes.shape
    a, b = np.triu_indices(G)                                                    # row-major over a <= b: the pair index
    e = np.concatenate([emit.astype(LD), np.ones((n, 2, 1), dtype=LD)], axis=2)[np.arange(n)[:, None], :, CLASS[codes[:, a], codes[:, b]]]
    rho = carry.astype(LD)
    rho[0] = 0
    prior = np.array([1 - LD(PI), LD(PI)])
    alpha, loglik, f = np.empty((n, len(a), 2), dtype=LD), np.zeros(len(a), dtype=LD), np.tile(prior, (len(a), 1))
    for i in range(n):
        f = e[i] * (rho[i] * f + (1 - rho[i]) * prior * f.sum(axis=1, keepdims=True))
        scale = f.sum(axis=1, keepdims=True)
        loglik += np.log(scale[:, 0])
        alpha[i] = f = f / scale
    beta, ibd = np.ones((len(a), 2), dtype=LD), np.zeros(len(a), dtype=LD)
    for i in range(n - 1, -1, -1):
        posterior = alpha[i] * beta
        ibd += (1 if weight is None else LD(weight[i])) * posterior[:, 1] / posterior.sum(axis=1)
        if i:
            back = e[i] * beta
            beta = rho[i] * back + (1 - rho[i]) * (back * prior).sum(axis=1, keepdims=True)
            beta /= beta.sum(axis=1, keepdims=True)
    want = np.stack([loglik, ibd], axis=1)
    want.setflags(write=False)
    return want


def run(kgx, *key, mask=None):
    codes, rows, emit, carry, weight = inputs(*key)
    pop = kgx.Population(key[0], V)
    pop.load_dosage2(kgx.pack_dosage2(codes_of(key[0])))
    if mask is not None:
        pop.set_genome_mask(mask)
    got = pop.pair_hmm(emit, carry, rows, key[1], weight, PI)
    pop.close()
    return got


def check(kgx, *key):
    got, want, n = run(kgx, *key), expected(*key), key[1]
    d = np.abs(got.astype(LD) - want)
    print("worst loglik error / bound", (d[:, 0] / (16 * n * U + 4 * U * np.abs(want[:, 0]))).max(), "ibd", (d[:, 1] / (32 * n * U * want[:, 1])).max())
    assert got.dtype == np.float64 and got.shape == want.shape and np.isfinite(got).all()
    assert (d[:, 0] <= 16 * n * U + 4 * U * np.abs(want[:, 0])).all() and (d[:, 1] <= 32 * n * U * want[:, 1]).all()
    return got


@pytest.mark.parametrize("listed", [False, True])
@pytest.mark.parametrize("n_rows", [1, 15, 16, 17, 64, 65, 513, 1100])
@pytest.mark.parametrize("G", [20, 33, 70])
def test_every_pair_equals_forward_backward(kgx, G, n_rows, listed):
    check(kgx, G, n_rows, listed)


@pytest.mark.parametrize("weighted,emit_value", [(True, None), (False, 2.0 ** -30), (False, 2.0 ** 30)])
def test_weights_and_the_ends_of_the_emission_range(kgx, weighted, emit_value):
    """1100 rows of 2^-30 or 2^30 leave the double range 65 times over: the shared exponent carries them."""
    assert np.abs(check(kgx, 70, V, False, weighted, emit_value)[:, 0]).max() > (1022 * np.log(2) if emit_value else 0)


def test_from_the_reference_alone():
    """Genomes 0 and 1 are identical and IBD nearly everywhere; two random genomes nearly nowhere."""
    share = expected(70, V, False)[:, 1] / V
    assert share[1] > 0.9 > share[5 * 70 - 5 * 4 // 2 + 1] and share[5 * 70 - 5 * 4 // 2 + 1] < 0.1           # pairs (0, 1) and (5, 6)


def test_genome_mask(kgx):
    keep = (np.arange(70) % 7 != 0).astype(np.uint8)
    a, b = np.triu_indices(70)
    both = (keep[a] & keep[b]).astype(bool)
    got, plain = run(kgx, 70, 400, False, mask=keep), run(kgx, 70, 400, False)
    assert not got[~both].any() and np.array_equal(got[both], plain[both]) and plain[~both, 1].all()


def test_one_device_listed_three_times(kgx):
    plain = run(kgx, 70, 400, True)
    try:
        kgx.init([0, 0, 0])
        assert np.array_equal(run(kgx, 70, 400, True), plain)
    finally:
        kgx.init(0)


@pytest.mark.parametrize("cap,batches", [("64", 7), ("128", 4), ("100", 4)])
def test_batches_change_no_bit(kgx, monkeypatch, cap, batches):
    """KGX_PAIR_HMM_ROWS=64: a batch a tile, the state carried by the table over every tile edge; 100 is rounded up to 128."""
    plain = check(kgx, 70, 400, False)
    monkeypatch.setenv("KGX_PAIR_HMM_ROWS", cap)
    kgx.reload_options()
    try:
        got = run(kgx, 70, 400, False)
        ms, reported = kgx.pair_hmm_last()
    finally:
        monkeypatch.delenv("KGX_PAIR_HMM_ROWS")
        kgx.reload_options()
    assert reported == batches and ms > 0.0 and np.array_equal(got, plain)


def test_refusals_and_the_empty_list(kgx):
    _, _, emit, carry, _ = inputs(33, V, False)
    pop = kgx.Population(33, V)
    pop.load_dosage2(kgx.pack_dosage2(codes_of(33)))
    out = np.ones((33 * 34 // 2, 2))

    def refused(message, rows=None, n_rows=V, emit=emit, carry=carry, weight=None, pi=PI, o=out, handle=pop._h):
        p, arrays = np.array([pi]), [rows, emit, carry, weight]
        rows, emit, carry, weight = (None if x is None else kgx.ptr(np.ascontiguousarray(x)) for x in arrays)
        rc = kgx.lib().kgx_pair_hmm(handle, rows, n_rows, emit, carry, weight, kgx.ptr(p), None if o is None else kgx.ptr(o))
        return rc == kgx.KGX_EINVAL and message in kgx.lib().kgx_last_error().decode()

    def changed(array, index, value):
        array = array.copy()
        array.flat[index] = value
        return array

    for value in (np.nan, np.inf, 2.0 ** -31, 2.0 ** 31, -1.0):
        assert refused("emit[7][1][2]", emit=changed(emit, 7 * 12 + 6 + 2, value))
    assert refused("carry[9]", carry=changed(carry, 9, 1.5)) and refused("carry[9]", carry=changed(carry, 9, np.nan))
    for value in (-1.0, np.inf, 2.0 ** 33):
        assert refused("weight[3]", weight=changed(np.ones(V), 3, value))
    assert refused("pi", pi=0.0) and refused("pi", pi=1.0) and refused("pi", pi=np.nan)
    assert refused("rows[1]", rows=np.array([5, V], dtype=np.uint32), n_rows=2)
    assert refused("n_rows", n_rows=V + 1) and refused("n_rows", n_rows=1 << 32)
    assert refused("null", emit=None) and refused("null", carry=None) and refused("null", o=None) and refused("null", handle=None)
    assert not refused("") and out[:, 1].all()                                        # ... and the call itself goes through
    assert not refused("", n_rows=0, emit=None, carry=None) and not out.any()         # n_rows == 0: {0, 0}, and nothing is needed
    pop.close()
