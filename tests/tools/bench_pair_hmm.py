"""kgx_pair_hmm on the synthetic biallelic population (kgx_population_synth_biallelic), all rows in position order, one batch:
python tests/tools/bench_pair_hmm.py [rows [genomes ...]]            (default: 100 000 rows; 2 504 and 10 000 genomes)

Prints per shape the device time of k_pair_hmm (HIP events, best of 3 after a call that grows the arena), the steps of the recursion
per second (G (G + 1) / 2 pairs x rows) and the fp64 issue slots per second they stand for (15 a step), and -- the yardsticks --
k_pair_counts' product time and k_pair_runs' walk time (IDENTICAL, min_sites 1) over the same rows and genomes."""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
GENOMES = [int(a) for a in sys.argv[2:]] or [2_504, 10_000]
FP64_SLOTS = 15                                                        # 2 adds, 8 multiplies, 5 fused multiply-adds a step

capi.ensure_built()
capi.init(0)

report = []
position = np.arange(1, N_ROWS + 1, dtype=np.uint32) * 230             # one contig, a site every 230 bases
carry = capi.ibd_carry(position, 1e-4)
for G in GENOMES:
    pop = capi.Population(G, N_ROWS)
    pop.synth_biallelic(1111, 0, 0)
    emit = capi.ibd_tables(pop.allele_count_by_locus()[:N_ROWS, :4], 1e-3)
    pairs = G * (G + 1) // 2
    counts = np.zeros((pairs, 9), dtype=np.uint32)
    product, runs, walk = [], [], []
    for _ in range(4):                                                 # the first call grows the arena: not counted
        capi.check(capi.lib().kgx_pair_counts(pop.handle, None, N_ROWS, capi.ptr(counts)))
        product.append(capi.pair_counts_last()[0])
    del counts
    for _ in range(4):
        pop.pair_runs(position, None, N_ROWS, None, 1, 1, 0, capi.KGX_SHARE_IDENTICAL)
        runs.append(capi.pair_runs_last()[0])
    for _ in range(4):
        table = pop.pair_hmm(emit, carry, None, N_ROWS, None, 0.5)
        ms, batches = capi.pair_hmm_last()
        walk.append(ms)
    product_ms, runs_ms, walk_ms = min(product[1:]), min(runs[1:]), min(walk[1:])
    steps = pairs * N_ROWS
    entry = {"genomes": G, "rows": N_ROWS, "walk_ms": round(walk_ms, 3), "row_batches": batches, "steps": steps,
             "steps_per_s": round(steps / (walk_ms * 1e-3), 0), "fp64_slots_per_s": round(FP64_SLOTS * steps / (walk_ms * 1e-3), 0),
             "pair_counts_product_ms": round(product_ms, 3), "pair_runs_walk_ms": round(runs_ms, 3), "walk_over_product": round(walk_ms / product_ms, 3),
             "walk_over_runs": round(walk_ms / runs_ms, 3), "mean_loglik": float(table[:, 0].mean()), "mean_ibd_share": float(table[:, 1].mean() / N_ROWS)}
    report.append(entry)
    print(f"{G} genomes x {N_ROWS} rows: walk {walk_ms:.2f} ms ({entry['steps_per_s']:.3g} steps/s, {entry['fp64_slots_per_s']:.3g} fp64 slots/s, "
          f"{batches} batch(es)); pair_counts product {product_ms:.2f} ms; pair_runs walk {runs_ms:.2f} ms; mean IBD share {entry['mean_ibd_share']:.4f}", flush=True)
    del table
    pop.close()
print(json.dumps(report))
