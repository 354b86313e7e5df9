"""kgx_roh on the synthetic biallelic population (kgx_population_synth_biallelic), all rows in position order, max_gap = 0:
python tests/tools/bench_roh.py [rows [genomes ...]]          (default: 1 000 000 rows; 2 504 and 10 000 genomes)

Prints per shape the device time of the count pass's walk, k_roh<false> (the library's own HIP events, best of 3 after one call
that grows the arena) -- at min_sites 100, where the runs between two hets of one tile are passed over, and at min_sites 1, where
each is looked at (four cells in ten of this population are non-zero: far denser than called variants) -- the algorithmic bytes
n_rows x ceil(G/4) over the former time and their share of the 8 TB/s HBM peak, and the wall time of the whole summaries-only call.  The yardstick is the count pass of kgx_genome_row_lists over the same rows: the same bytes
in the same walk with one butterfly a tile instead of two and no run machine.  The library keeps no timer for that kernel, so its
sizing call is timed here by the wall clock (allocations and the small kernels included) and the two kernels are compared by a
kernel trace of this script (profiles/roh.md says how)."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

N_ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
GENOMES = [int(a) for a in sys.argv[2:]] or [2_504, 10_000]
HBM_PEAK = 8e12                          # MI355X: 8 TB/s

capi.ensure_built()
capi.init(0)

position = (np.arange(N_ROWS, dtype=np.uint64) * 100 + 1).astype(np.uint32)      # 100 bases a row: below 2^32 up to 42 M rows
report = []
for G in GENOMES:
    pop = capi.Population(G, N_ROWS)
    pop.synth_biallelic(1111, 0, 0)
    walk, walls = {100: [], 1: []}, []
    for _ in range(4):                                                           # the first call grows the arena: not counted
        t0 = time.perf_counter()
        summary, _, _ = pop.roh(position, min_sites=100, min_length=5000, runs=False)
        walls.append(time.perf_counter() - t0)
        ms, slices = capi.roh_last()
        walk[100].append(ms)
        pop.roh(position, min_sites=1, min_length=5000, runs=False)              # every run between two hets of a tile is looked at
        walk[1].append(capi.roh_last()[0])
    begin = np.zeros(G + 1, dtype=np.uint64)
    lists = []
    for _ in range(4):
        t0 = time.perf_counter()
        capi.check(capi.lib().kgx_genome_row_lists(pop.handle, 0, G, None, capi.ptr(begin), None, 0))
        lists.append(time.perf_counter() - t0)
    walk_ms, matrix_bytes = min(walk[100][1:]), N_ROWS * ((G + 3) // 4)
    entry = {"genomes": G, "rows": N_ROWS, "walk_ms": round(walk_ms, 3), "walk_ms_min_sites_1": round(min(walk[1][1:]), 3), "row_slices": slices, "bytes": matrix_bytes,
             "bytes_per_s": round(matrix_bytes / (walk_ms * 1e-3), 0), "share_of_hbm_peak": round(matrix_bytes / (walk_ms * 1e-3) / HBM_PEAK, 4),
             "call_wall_ms": round(min(walls[1:]) * 1e3, 2), "row_lists_sizing_call_wall_ms": round(min(lists[1:]) * 1e3, 2),
             "runs": int(summary["runs"].sum()), "row_list_entries": int(begin[G])}
    report.append(entry)
    print(f"{G} genomes x {N_ROWS} rows: walk {walk_ms:.3f} ms at min_sites 100, {entry['walk_ms_min_sites_1']:.3f} ms at 1, in {slices} slices "
          f"({entry['bytes_per_s'] / 1e12:.2f} TB/s, {entry['share_of_hbm_peak']:.1%} of HBM peak); "
          f"summaries-only call {entry['call_wall_ms']:.2f} ms; row lists' sizing call {entry['row_lists_sizing_call_wall_ms']:.2f} ms by the wall clock", flush=True)
    pop.close()
print(json.dumps(report))
