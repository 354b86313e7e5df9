"""kgx_pair_scores with GRM tables on the synthetic biallelic population (kgx_population_synth_biallelic), all rows:
python tests/tools/bench_pair_scores.py [rows [genomes ...]]          (default: 100 000 rows; 2 504 and 10 000 genomes)

Prints per shape the device time of the product kernel (HIP events, best of 3) and its multiply-accumulates 4 x G (G + 1) / 2 x
n_rows over that time; beside it kgx_pair_counts' product kernel over the same rows in the same run, and -- the yardstick outside
the library -- torch on the same device: Z @ Z.T of the fp16 matrix of the same quantised z with fp32 accumulation.  The largest
difference between the two GRMs is reported, not asserted: fp16 rounds z to 11 bits and fp32 rounds the sums; the kernel does neither."""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
GENOMES = [int(a) for a in sys.argv[2:]] or [2_504, 10_000]
MIN_MAF = 0.01

capi.ensure_built()
capi.init(0)
import torch  # noqa: E402  (after capi: one HIP runtime in the process)

dev = torch.device("cuda:0")


def timed(fn, repeats=3):
    """(best ms of `repeats` after one warm-up, the last result)"""
    result, best = fn(), float("inf")
    for _ in range(repeats):
        del result
        torch.cuda.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        result = fn()
        end.record()
        torch.cuda.synchronize()
        best = min(best, begin.elapsed_time(end))
    return best, result


report = []
for G in GENOMES:
    pop = capi.Population(G, N_ROWS)
    pop.synth_biallelic(1111, 0, 0)
    tables, scale_bits, rows_used = capi.grm_tables(pop.allele_count_by_locus(), MIN_MAF)
    scores = np.zeros(G * (G + 1) // 2, dtype=np.int64)
    counts = np.zeros((G * (G + 1) // 2, 9), dtype=np.uint32)
    scores_ms, counts_ms = [], []
    for _ in range(4):                                                     # the first call grows the arena: not counted
        capi.check(capi.lib().kgx_pair_scores(pop.handle, None, N_ROWS, capi.ptr(tables), capi.ptr(scores)))
        ms, batches, splits = capi.pair_scores_last()
        scores_ms.append(ms)
        capi.check(capi.lib().kgx_pair_counts(pop.handle, None, N_ROWS, capi.ptr(counts)))
        counts_ms.append(capi.pair_counts_last()[0])
    product_ms, pair_counts_ms = min(scores_ms[1:]), min(counts_ms[1:])
    grm = capi.grm_finish(scores, G, scale_bits, rows_used)
    macs = 4 * (G * (G + 1) // 2) * N_ROWS

    packed = torch.from_numpy(pop.read_dosage2()).to(dev)                  # [n_rows][ceil(G / 4)]
    z_of_code = (torch.from_numpy(tables).to(dev).to(torch.float32) / float(2 ** scale_bits)).to(torch.float16)
    Z = torch.empty((G, N_ROWS), dtype=torch.float16, device=dev)
    for r0 in range(0, N_ROWS, 8192):
        codes = torch.stack([(packed[r0:r0 + 8192] >> s) & 3 for s in (0, 2, 4, 6)], dim=2).reshape(-1, packed.shape[1] * 4)[:, :G]
        Z[:, r0:r0 + 8192] = torch.gather(z_of_code[r0:r0 + 8192], 1, codes.to(torch.int64)).T
    mm_ms, P = timed(lambda: torch.mm(Z, Z.T, out_dtype=torch.float32))
    a, b = np.triu_indices(G)
    torch_grm = (P.cpu().numpy()[a, b].astype(np.float64)) / rows_used
    del Z, P, packed, codes
    pop.close()
    entry = {"genomes": G, "rows": N_ROWS, "rows_used": rows_used, "scale_bits": scale_bits, "product_ms": round(product_ms, 3), "row_batches": batches,
             "row_splits": splits, "product_macs": macs, "product_macs_per_s": round(macs / (product_ms * 1e-3), 0),
             "pair_counts_product_ms": round(pair_counts_ms, 3), "product_over_pair_counts": round(product_ms / pair_counts_ms, 3),
             "torch_fp16_product_ms": round(mm_ms, 3), "product_over_torch_product": round(product_ms / mm_ms, 3),
             "largest_difference_from_torch": float(np.max(np.abs(grm - torch_grm)))}
    report.append(entry)
    print(f"{G} genomes x {N_ROWS} rows (scale 2^{scale_bits}, {rows_used} used): product {product_ms:.2f} ms ({entry['product_macs_per_s']:.3g} MAC/s, {batches} "
          f"batch(es), {splits} slice(s)); pair_counts product {pair_counts_ms:.2f} ms; torch fp16 Z @ Z.T {mm_ms:.2f} ms; largest difference "
          f"{entry['largest_difference_from_torch']:.3g}", flush=True)
print(json.dumps(report))
