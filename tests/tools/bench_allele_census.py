"""kgx_gt8_allele_census on the synthetic multi-allelic population (kgx_gt8_synth_multiallelic), 10 000 genomes x 1 000 000 loci:
python tests/tools/bench_allele_census.py [genomes loci [groups,amax ...]]          (default shapes: 6,3 32,3 6,1 6,14)

Prints per shape the census kernel's device time (kgx_gt8_allele_census_last, best of 3) with its algorithmic bytes
(n_selected x G + G + 4 x (3 + 2 amax) x n_groups x n_selected), and -- the yardstick -- kgx_inbreed_last_kernel_ms of a
KGX_ALGO_SIMPLE call over the same matrix and all loci: the existing kernel that reads the same bytes, on the same build."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

G = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
L = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
SHAPES = [tuple(int(x) for x in s.split(",")) for s in sys.argv[3:]] or [(6, 3), (32, 3), (6, 1), (6, 14)]

capi.ensure_built()
capi.init(0)
m = capi.GenotypeMatrix(G, L)
table = m.synth_multiallelic(1111, 0, 0)

yard = []
for _ in range(3):
    m.inbreed(table, "Simple", phased=True)
    yard.append(capi.inbreed_last_kernel_ms())
yard_ms = min(yard)
sweep_bytes = int(capi.lib().kgx_gt8_sweep_bytes(G, L, 3))

result = {"genomes": G, "loci": L, "simple_sweep_kernel_ms": round(yard_ms, 3), "simple_sweep_bytes": sweep_bytes,
          "simple_sweep_GBps": round(sweep_bytes / (yard_ms * 1e-3) / 1e9, 1) if yard_ms > 0 else None, "census": []}
for n_groups, amax in SHAPES:
    groups = (np.arange(G) % (n_groups + 1)).astype(np.uint8)
    groups[groups == n_groups] = 0xFF                                  # one genome in n_groups + 1 is in no group
    out = np.zeros((L, n_groups, 3 + 2 * amax), dtype=np.uint32)
    kernels, walls, batches = [], [], 0
    for _ in range(3):
        t0 = time.perf_counter()
        capi.check(capi.lib().kgx_gt8_allele_census(m._h, capi.ptr(groups), n_groups, None, L, amax, capi.ptr(out)))
        walls.append(time.perf_counter() - t0)
        ms, batches = capi.allele_census_last()
        kernels.append(ms)
    kernel_ms = min(kernels)
    algorithmic = L * G + G + 4 * (3 + 2 * amax) * n_groups * L
    result["census"].append({"n_groups": n_groups, "amax": amax, "kernel_ms": round(kernel_ms, 3), "batches": batches, "algorithmic_bytes": algorithmic,
                             "kernel_GBps": round(algorithmic / (kernel_ms * 1e-3) / 1e9, 1) if kernel_ms > 0 else None,
                             "ratio_to_simple_sweep": round(kernel_ms / yard_ms, 2) if yard_ms > 0 else None, "call_wall_ms": round(min(walls) * 1e3, 1),
                             "copies_counted": int(out[:, :, 3::2].sum(dtype=np.uint64) + 2 * out[:, :, 4::2].sum(dtype=np.uint64))})
    print(f"census {n_groups} groups, amax {amax}: kernel {kernel_ms:.2f} ms over {algorithmic / 1e9:.2f} GB in {batches} batch(es); "
          f"Simple sweep kernel {yard_ms:.2f} ms: ratio {kernel_ms / yard_ms if yard_ms > 0 else float('nan'):.2f}", flush=True)
print(json.dumps(result))
m.close()
