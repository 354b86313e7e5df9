"""kgx_pair_runs on the synthetic biallelic population (kgx_population_synth_biallelic), all rows in position order, one batch:
python tests/tools/bench_pair_runs.py [rows [genomes ...]]            (default: 100 000 rows; 2 504 and 10 000 genomes)

Prints per shape, mode (IBS0, IDENTICAL) and min_sites (1, 100) the device time of k_pair_runs (HIP events, best of 3 after a call
that grows the arena), the pair-tiles walked per second (G (G + 1) / 2 pairs x ceil(rows / 64) tiles) and -- the yardstick --
k_pair_counts' product time over the same rows and genomes (kgx_pair_counts_last), with the ratio of the two."""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
GENOMES = [int(a) for a in sys.argv[2:]] or [2_504, 10_000]

capi.ensure_built()
capi.init(0)

report = []
position = np.arange(1, N_ROWS + 1, dtype=np.uint32) * 230             # one contig, a site every 230 bases
for G in GENOMES:
    pop = capi.Population(G, N_ROWS)
    pop.synth_biallelic(1111, 0, 0)
    pairs = G * (G + 1) // 2
    counts = np.zeros((pairs, 9), dtype=np.uint32)
    product = []
    for _ in range(4):                                                 # the first call grows the arena: not counted
        capi.check(capi.lib().kgx_pair_counts(pop.handle, None, N_ROWS, capi.ptr(counts)))
        product.append(capi.pair_counts_last()[0])
    product_ms, count_batches = min(product[1:]), capi.pair_counts_last()[1]
    del counts
    pair_tiles = pairs * ((N_ROWS + 63) // 64)
    for mode, name in ((capi.KGX_SHARE_IBS0, "IBS0"), (capi.KGX_SHARE_IDENTICAL, "IDENTICAL")):
        for min_sites in (1, 100):
            walk = []
            for _ in range(4):
                table = pop.pair_runs(position, None, N_ROWS, None, min_sites, 1, 0, mode)
                ms, batches = capi.pair_runs_last()
                walk.append(ms)
            walk_ms = min(walk[1:])
            entry = {"genomes": G, "rows": N_ROWS, "mode": name, "min_sites": min_sites, "walk_ms": round(walk_ms, 3), "row_batches": batches,
                     "pair_tiles": pair_tiles, "pair_tiles_per_s": round(pair_tiles / (walk_ms * 1e-3), 0), "pair_counts_product_ms": round(product_ms, 3),
                     "pair_counts_row_batches": count_batches, "walk_over_product": round(walk_ms / product_ms, 3),
                     "runs": int(table[:, 0].sum()), "longest": int(table[:, 2].max())}
            report.append(entry)
            print(f"{G} genomes x {N_ROWS} rows, {name}, min_sites {min_sites}: walk {walk_ms:.2f} ms ({entry['pair_tiles_per_s']:.3g} pair-tiles/s, "
                  f"{batches} batch(es)); pair_counts product {product_ms:.2f} ms; ratio {entry['walk_over_product']:.2f}; {entry['runs']} runs", flush=True)
            del table
    pop.close()
print(json.dumps(report))
