"""kgx_ld_counts on the synthetic biallelic population (kgx_population_synth_biallelic), all rows in position order:
python tests/tools/bench_ld_counts.py [rows [genomes ...]]          (default: 100 000 rows; 2 504 and 10 000 genomes; windows 64, 512)

Prints per shape the device time of the product kernel (HIP events, best of 3), the multiply-accumulates the table stands for,
9 x n_rows x (window + 1) x G, over that time as a share of the device's dense int8 peak, and -- the yardstick, outside the
library -- torch on the same device doing the same band by blocks: Z [n_rows][3][G] fp16 from the same codes, cut into blocks of
K = max(window, 64) rows, and per block Z_A @ Z_B.T with fp32 accumulation (exact up to 2^24), Z_B the block and the next one (one
batched product; it computes a 2 K wide rectangle per row where the band needs window + 1).  Building Z and the product are timed
each on its own.  The torch band must equal the kernel's table, word for word."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
GENOMES = [int(a) for a in sys.argv[2:]] or [2_504, 10_000]
WINDOWS = [64, 512]
INT8_PEAK_MACS = 2.5e15                # MI355X: 5 POPS dense int8 (two operations a multiply-accumulate)

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
    packed = torch.from_numpy(pop.read_dosage2()).to(dev)                  # [n_rows][ceil(G / 4)]
    kinds = torch.tensor([1, 2, 3], dtype=torch.uint8, device=dev).view(1, 3, 1)
    for window in WINDOWS:
        out = np.zeros((N_ROWS, window + 1, 9), dtype=np.uint32)
        product, walls = [], []
        for _ in range(4):                                                 # the first call grows the arena: not counted
            t0 = time.perf_counter()
            capi.check(capi.lib().kgx_ld_counts(pop.handle, None, N_ROWS, window, capi.ptr(out)))
            walls.append(time.perf_counter() - t0)
            ms, batches, splits = capi.ld_counts_last()
            product.append(ms)
        product_ms = min(product[1:])
        macs = 9 * N_ROWS * (window + 1) * G

        K = max(window, 64)
        blocks = (N_ROWS + K - 1) // K

        def build():
            codes = torch.stack([(packed >> s) & 3 for s in (0, 2, 4, 6)], dim=2).reshape(N_ROWS, -1)[:, :G]
            Z = torch.zeros(((blocks + 1) * K, 3, G), dtype=torch.float16, device=dev)       # the rows past the list are code 0
            Z[:N_ROWS] = codes.unsqueeze(1) == kinds
            A = Z.view(blocks + 1, 3 * K, G)                                                  # row 3 o + kind of block b
            return A[:blocks], torch.cat([A[:blocks], A[1:]], dim=1)                          # Z_B: the block and the next one

        build_ms, (ZA, ZB) = timed(build)
        mm_ms, P = timed(lambda: torch.bmm(ZA, ZB.transpose(1, 2), out_dtype=torch.float32))
        o = torch.arange(K, device=dev).view(K, 1)
        d = torch.arange(window + 1, device=dev).view(1, window + 1)
        band = P.view(blocks, K, 3, 2 * K, 3).permute(0, 1, 3, 2, 4)[:, o, o + d]             # [block][o][d][p][q]
        band = band.reshape(blocks * K, window + 1, 9)[:N_ROWS].to(torch.int32)
        same = bool(torch.equal(band, torch.from_numpy(out.view(np.int32)).to(dev)))          # counts <= G < 2^31
        del ZA, ZB, P, band
        entry = {"genomes": G, "rows": N_ROWS, "window": window, "product_ms": round(product_ms, 3), "row_batches": batches, "genome_splits": splits,
                 "call_wall_ms": round(min(walls[1:]) * 1e3, 1), "table_macs": macs, "table_macs_per_s": round(macs / (product_ms * 1e-3), 0),
                 "share_of_int8_peak": round(macs / (product_ms * 1e-3) / INT8_PEAK_MACS, 4), "table_bytes": out.nbytes, "torch_block_rows": K,
                 "torch_build_ms": round(build_ms, 3), "torch_product_ms": round(mm_ms, 3), "product_over_torch_product": round(product_ms / mm_ms, 3),
                 "torch_equals_kernel": same}
        report.append(entry)
        print(f"{G} genomes x {N_ROWS} rows, window {window}: product {product_ms:.2f} ms ({entry['share_of_int8_peak']:.1%} of int8 peak, {batches} batch(es), "
              f"{splits} slice(s)); torch build {build_ms:.2f} ms + product {mm_ms:.2f} ms; equal: {same}", flush=True)
        if not same:
            raise SystemExit("the torch band differs from kgx_ld_counts")
    del packed
    pop.close()
print(json.dumps(report))
