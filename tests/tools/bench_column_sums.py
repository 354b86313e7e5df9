"""kgx_column_sums with trait columns on the synthetic biallelic population (kgx_population_synth_biallelic), all rows:
python tests/tools/bench_column_sums.py [rows [genomes [traits ...]]]      (default: 100 000 rows, 10 000 genomes; 1, 16 and 32 traits)

Prints per trait count the device time of the product kernel (HIP events, best of 3 after a call that grows the arena) and its
multiply-accumulates 3 x n_rows x n_columns x G over that time.  Beside it (a) the by-locus count sweep over the same rows -- the
floor of reading them once -- and (b) the yardstick outside the library, torch on the same device: the three fp16 indicator
matrices (built beforehand, not timed) times the fp16 columns with fp32 accumulation, one matrix product.  The kernel's table is
checked for equality against an fp64 product of the first 4 096 rows (exact: every sum is below 2^53); the fp16 product is only
timed -- fp16 cannot hold a 14-bit q, let alone q^2."""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
G = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000
TRAITS = [int(a) for a in sys.argv[3:]] or [1, 16, 32]
CHECKED = min(N_ROWS, 4096)

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


pop = capi.Population(G, N_ROWS)
pop.synth_biallelic(1111, 0, 0)
scratch = torch.empty((N_ROWS, 4), dtype=torch.int32, device=dev)
sweep_ms = float(np.median(pop.allele_count_timed(scratch.data_ptr(), torch.cuda.current_stream().cuda_stream, 2, 10)))
del scratch
packed = torch.from_numpy(pop.read_dosage2()).to(dev)                      # [n_rows][ceil(G / 4)]
Z = torch.empty((3, N_ROWS, G), dtype=torch.float16, device=dev)
for r0 in range(0, N_ROWS, 8192):
    codes = torch.stack([(packed[r0:r0 + 8192] >> s) & 3 for s in (0, 2, 4, 6)], dim=2).reshape(-1, packed.shape[1] * 4)[:, :G]
    for k in range(3):
        Z[k, r0:r0 + 8192] = codes == k + 1
del packed, codes

report = []
for traits in TRAITS:
    y = np.random.default_rng(traits).normal(size=(traits, G))
    columns, scale_bits = capi.assoc_columns(y)
    C = len(columns)
    out = np.zeros((N_ROWS, C, 3), dtype=np.int64)
    product_ms = []
    for _ in range(4):                                                     # the first call grows the arena: not counted
        capi.check(capi.lib().kgx_column_sums(pop.handle, None, N_ROWS, capi.ptr(columns), C, capi.ptr(out)))
        ms, batches, splits = capi.column_sums_last()
        product_ms.append(ms)
    product_ms = min(product_ms[1:])
    exact = torch.einsum("kig,jg->ijk", Z[:, :CHECKED].to(torch.float64), torch.from_numpy(columns).to(dev).to(torch.float64))
    equal = bool(np.array_equal(exact.cpu().numpy().astype(np.int64), out[:CHECKED]))
    W = (torch.from_numpy(columns).to(dev).to(torch.float32) / 8192.0).to(torch.float16).T.contiguous()     # [G][C]
    mm_ms = timed(lambda: torch.mm(Z.reshape(3 * N_ROWS, G), W, out_dtype=torch.float32))
    del exact, W
    macs = 3 * N_ROWS * C * G
    entry = {"genomes": G, "rows": N_ROWS, "traits": traits, "columns": C, "scale_bits": scale_bits, "product_ms": round(product_ms, 3), "row_batches": batches,
             "genome_splits": splits, "product_macs": macs, "product_macs_per_s": round(macs / (product_ms * 1e-3), 0), "row_bytes_per_s": round(pop.sweep_bytes / (product_ms * 1e-3), 0),
             "by_locus_sweep_ms": round(sweep_ms, 3), "product_over_sweep": round(product_ms / sweep_ms, 3), "torch_fp16_product_ms": round(mm_ms, 3),
             "product_over_torch_product": round(product_ms / mm_ms, 3), "first_rows_equal_fp64_product": equal}
    report.append(entry)
    print(f"{traits} trait(s) = {C} columns x {G} genomes x {N_ROWS} rows (scale 2^{scale_bits}): product {product_ms:.3f} ms ({entry['product_macs_per_s']:.3g} MAC/s, "
          f"{batches} batch(es), {splits} slice(s)); by-locus sweep {sweep_ms:.3f} ms; torch fp16 indicators @ columns {mm_ms:.3f} ms; first {CHECKED} rows equal: {equal}",
          flush=True)
pop.close()
print(json.dumps(report))
