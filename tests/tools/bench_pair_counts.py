"""kgx_pair_counts on the synthetic biallelic population (kgx_population_synth_biallelic), all rows:
python tests/tools/bench_pair_counts.py [rows [genomes ...]]          (default: 100 000 rows; 2 504 and 10 000 genomes)

Prints per shape the device times of the two stages (panel kernels, product kernel: HIP events, best of 3), the product's
multiply-accumulates 9 x G (G + 1) / 2 x n_rows over its time as a share of the device's dense int8 peak, and -- the yardstick,
outside the library -- torch on the same device: building Z [3 G][n_rows] fp16 from the same codes, and Z @ Z.T with fp32
accumulation (exact up to 2^24), each timed on its own.  The torch result must equal the kernel's, word for word."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
GENOMES = [int(a) for a in sys.argv[2:]] or [2_504, 10_000]
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
    out = np.zeros((G * (G + 1) // 2, 9), dtype=np.uint32)
    panel, product, walls = [], [], []
    for _ in range(4):                                                     # the first call grows the arena: not counted
        t0 = time.perf_counter()
        capi.check(capi.lib().kgx_pair_counts(pop.handle, None, N_ROWS, capi.ptr(out)))
        walls.append(time.perf_counter() - t0)
        ms, batches, splits = capi.pair_counts_last()
        product.append(ms)
        panel.append(capi.pair_counts_last_panel_ms())
    panel_ms, product_ms = min(panel[1:]), min(product[1:])
    macs = 9 * (G * (G + 1) // 2) * N_ROWS

    packed = torch.from_numpy(pop.read_dosage2()).to(dev)                  # [n_rows][ceil(G / 4)]
    kinds = torch.tensor([1, 2, 3], dtype=torch.uint8, device=dev).view(1, 3, 1)

    def build():
        codes = torch.stack([(packed >> s) & 3 for s in (0, 2, 4, 6)], dim=2).reshape(N_ROWS, -1)[:, :G]
        return (codes.T.unsqueeze(1) == kinds).reshape(3 * G, N_ROWS).to(torch.float16)     # row 3 g + kind

    build_ms, Z = timed(build)
    mm_ms, P = timed(lambda: torch.mm(Z, Z.T, out_dtype=torch.float32))
    a, b = torch.triu_indices(G, G, device=dev)
    same = bool(torch.equal(P.view(G, 3, G, 3).permute(0, 2, 1, 3)[a, b].reshape(-1, 9).to(torch.int32),
                            torch.from_numpy(out.view(np.int32)).to(dev)))              # counts <= n_rows < 2^31
    del Z, P, packed, a, b
    pop.close()
    entry = {"genomes": G, "rows": N_ROWS, "panel_ms": round(panel_ms, 3), "product_ms": round(product_ms, 3), "row_batches": batches, "row_splits": splits,
             "call_wall_ms": round(min(walls[1:]) * 1e3, 1), "product_macs": macs, "product_macs_per_s": round(macs / (product_ms * 1e-3), 0),
             "share_of_int8_peak": round(macs / (product_ms * 1e-3) / INT8_PEAK_MACS, 4), "torch_build_ms": round(build_ms, 3),
             "torch_product_ms": round(mm_ms, 3), "product_over_torch_product": round(product_ms / mm_ms, 3),
             "both_stages_over_torch_both": round((panel_ms + product_ms) / (build_ms + mm_ms), 3), "torch_equals_kernel": same}
    report.append(entry)
    print(f"{G} genomes x {N_ROWS} rows: panel {panel_ms:.2f} ms + product {product_ms:.2f} ms ({entry['share_of_int8_peak']:.1%} of int8 peak, "
          f"{batches} batch(es), {splits} slice(s)); torch build {build_ms:.2f} ms + product {mm_ms:.2f} ms; equal: {same}", flush=True)
    if not same:
        raise SystemExit("the torch product differs from kgx_pair_counts")
print(json.dumps(report))
