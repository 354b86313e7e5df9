"""kgx_genome_scores with effect-size columns on the synthetic biallelic population (kgx_population_synth_biallelic), all rows:
python tests/tools/bench_genome_scores.py [rows [genomes [scores ...]]]      (default: 100 000 rows, 10 000 genomes; 1, 16 and 64 scores)

Prints per score count the device time of the product kernel (HIP events, best of 3 after a call that grows the arena) and its
multiply-accumulates as the digits run it, 3 x G x n_rows x 16 x tiles, over that time.  Beside it, in the same run, (a)
kgx_column_sums with the same number of two-digit columns (the transposed product, which needs no transposition of the codes), by
its own events and the same count, and (b) the yardstick outside the library, torch on the same device: the three fp16 indicator
matrices (built beforehand, not timed), transposed, times the fp16 weights with fp32 accumulation, and the largest deviation of that
product from the exact table.  The kernel's table is checked for equality against an fp64 product for the first 1 024 genomes
(exact: every sum is below 2^53)."""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
SCORES = [int(a) for a in sys.argv[3:]] or [1, 16, 64]
CHECKED = min(G, 1024)

capi.ensure_built()
capi.init(0)
import torch  # noqa: E402  (after capi: one HIP runtime in the process)

dev = torch.device("cuda:0")


def timed(fn, repeats=3):
    """best ms of `repeats` after one warm-up"""
    fn()
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        best = min(best, begin.elapsed_time(end))
    return best


def tiles_of(values):
    """the MFMA tiles of [C][n] values in groups of 16 columns: one digit where the whole group lies in [-64, 63], else two"""
    return sum(1 if (values[c:c + 16].min() >= -64 and values[c:c + 16].max() <= 63) else 2 for c in range(0, len(values), 16))


pop = capi.Population(G, N_ROWS)
pop.synth_biallelic(1111, 0, 0)
packed = torch.from_numpy(pop.read_dosage2()).to(dev)                      # [n_rows][ceil(G / 4)]
Z = torch.empty((3, N_ROWS, G), dtype=torch.float16, device=dev)
for r0 in range(0, N_ROWS, 8192):
    codes = torch.stack([(packed[r0:r0 + 8192] >> s) & 3 for s in (0, 2, 4, 6)], dim=2).reshape(-1, packed.shape[1] * 4)[:, :G]
    for k in range(3):
        Z[k, r0:r0 + 8192] = codes == k + 1
del packed, codes

report = []
for scores in SCORES:
    rng = np.random.default_rng(scores)
    weights, scale_bits = capi.score_weights(rng.normal(size=(scores, N_ROWS)))
    out = np.zeros((G, scores, 3), dtype=np.int64)
    product_ms = []
    for _ in range(4):                                                     # the first call grows the arena: not counted
        capi.check(capi.lib().kgx_genome_scores(pop.handle, None, N_ROWS, capi.ptr(weights), scores, capi.ptr(out)))
        ms, batches, splits = capi.genome_scores_last()
        product_ms.append(ms)
    product_ms = min(product_ms[1:])
    W64 = torch.from_numpy(weights).to(dev).to(torch.float64)
    exact = torch.einsum("kig,ji->gjk", Z[:, :, :CHECKED].to(torch.float64), W64).cpu().numpy().astype(np.int64)
    equal = bool(np.array_equal(exact, out[:CHECKED]))
    W = W64.to(torch.float16).T.contiguous()                               # [n_rows][C]: fp16 rounds a 14-bit weight to 11 bits
    mm_ms = timed(lambda: [torch.mm(Z[k].T, W, out_dtype=torch.float32) for k in range(3)])
    rounded = torch.stack([torch.mm(Z[k].T, W, out_dtype=torch.float32) for k in range(3)], dim=2).cpu().numpy()
    deviation = float(np.abs(rounded.astype(np.float64) - out).max())
    del exact, W, W64, rounded

    columns = capi.assoc_columns(rng.normal(size=(scores, G)))[0][:scores]    # q alone: two digits, as the weights
    sums = np.zeros((N_ROWS, scores, 3), dtype=np.int64)
    column_ms = []
    for _ in range(4):
        capi.check(capi.lib().kgx_column_sums(pop.handle, None, N_ROWS, capi.ptr(columns), scores, capi.ptr(sums)))
        column_ms.append(capi.column_sums_last()[0])
    column_ms = min(column_ms[1:])
    del sums

    tiles, column_tiles = tiles_of(weights), tiles_of(columns)
    macs, column_macs = 3 * G * N_ROWS * 16 * tiles, 3 * G * N_ROWS * 16 * column_tiles
    entry = {"genomes": G, "rows": N_ROWS, "scores": scores, "scale_bits": scale_bits, "tiles": tiles, "product_ms": round(product_ms, 3), "row_batches": batches,
             "row_splits": splits, "product_macs": macs, "product_macs_per_s": round(macs / (product_ms * 1e-3), 0), "column_sums_tiles": column_tiles,
             "column_sums_ms": round(column_ms, 3), "column_sums_macs_per_s": round(column_macs / (column_ms * 1e-3), 0),
             "macs_per_s_over_column_sums": round(macs / product_ms / (column_macs / column_ms), 3), "torch_fp16_product_ms": round(mm_ms, 3),
             "product_over_torch_product": round(product_ms / mm_ms, 3), "torch_fp16_largest_deviation": deviation, "first_genomes_equal_fp64_product": equal}
    report.append(entry)
    print(f"{scores} score(s) x {G} genomes x {N_ROWS} rows (scale 2^{scale_bits}, {tiles} tile(s)): product {product_ms:.3f} ms ({entry['product_macs_per_s']:.3g} MAC/s, "
          f"{batches} batch(es), {splits} slice(s)); column_sums {column_ms:.3f} ms ({entry['column_sums_macs_per_s']:.3g} MAC/s, {column_tiles} tile(s)); "
          f"torch fp16 indicators.T @ weights {mm_ms:.3f} ms, largest deviation {deviation:.6g}; first {CHECKED} genomes equal: {equal}", flush=True)
pop.close()
print(json.dumps(report))
