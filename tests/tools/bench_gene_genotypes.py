"""kgx_gene_genotypes on a synthetic 10 000 x 1 000 000 population with 5 000 disjoint genes of 100 rows (half the rows):
python tests/tools/bench_gene_genotypes.py [genomes variants genes rows_per_gene [empty]]
("empty": an all-reference population, every dword skipped -- what the sweep costs without its arithmetic)

Prints the hashing kernel's device time (kgx_gene_genotypes_last_ms) with its algorithmic bytes (member rows x ceil(G/4) + 8 B
per member + 24 B per (gene, genome)), the whole call's wall time, and -- the yardstick -- the time of
kgx_compound_offsets_listed over the same row lists: the existing kernel with the same access pattern."""
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from kgl_gene_amd import capi  # noqa: E402

G = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000
V = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
N_GENES = int(sys.argv[3]) if len(sys.argv) > 3 else 5_000
PER_GENE = int(sys.argv[4]) if len(sys.argv) > 4 else 100
EMPTY = len(sys.argv) > 5 and sys.argv[5] == "empty"      # nobody carries anything: every dword is skipped (the sweep's memory side alone)
assert N_GENES * PER_GENE <= V

capi.ensure_built()
capi.init(0)
pop = capi.Population(G, V)
if not EMPTY:
    pop.synth_biallelic(1111, 0, 0)
rng = np.random.default_rng(5)
key = rng.integers(0, 2**32, V, dtype=np.uint64)                      # CRC-32 sized keys, as the reference's
# disjoint genes: gene i = every (V / members)-th row from its own start, so the rows of a gene are not adjacent
members = (np.arange(N_GENES * PER_GENE, dtype=np.uint64) * (V // (N_GENES * PER_GENE))).astype(np.uint32)
first = (np.arange(N_GENES, dtype=np.uint32) * PER_GENE).astype(np.uint32)
n_rows = np.full(N_GENES, PER_GENE, dtype=np.uint32)
census = np.zeros(N_GENES, dtype=capi.GENE_CENSUS)
begin = np.zeros(N_GENES + 1, dtype=np.uint64)
args = (pop.handle, capi.ptr(key), capi.ptr(members), len(members), capi.ptr(first), capi.ptr(n_rows), N_GENES)

walls, kernels = [], []
for _ in range(3):
    t0 = time.perf_counter()
    capi.check(capi.lib().kgx_gene_genotypes(*args, None, None, capi.ptr(census), capi.ptr(begin), None, None, 0))
    walls.append(time.perf_counter() - t0)
    kernels.append(capi.gene_genotypes_last_ms())
kernel_ms, wall_ms = min(kernels), min(walls) * 1e3
algorithmic = len(members) * ((G + 3) // 4) + 8 * len(members) + 24 * N_GENES * G

bins = np.zeros(N_GENES, dtype=np.uint32)
yard = []
for _ in range(3):
    t0 = time.perf_counter()
    pop.compound_offsets_listed(members, first, n_rows, bins, 1)
    yard.append(time.perf_counter() - t0)
yard_ms = min(yard) * 1e3

result = {
    "genomes": G, "variants": V, "genes": N_GENES, "rows_per_gene": PER_GENE,
    "gene_genotypes_kernel_ms": round(kernel_ms, 3),
    "algorithmic_bytes": algorithmic,
    "kernel_GBps": round(algorithmic / (kernel_ms * 1e-3) / 1e9, 1) if kernel_ms > 0 else None,
    "gene_genotypes_call_wall_ms": round(wall_ms, 1),
    "compound_offsets_listed_call_wall_ms": round(yard_ms, 1),
    "genotypes_total": int(begin[-1]),
}
print(json.dumps(result))
print(f"hashing kernel {kernel_ms:.2f} ms over {algorithmic / 1e9:.2f} GB; whole call (K2 under the mask, sweep, census; sizing form) {wall_ms:.0f} ms; "
      f"yardstick kgx_compound_offsets_listed (whole call, same row lists) {yard_ms:.0f} ms")
pop.close()
