"""The carry-save counters of the by-genome sweep (kgl_gene_amd/csrc/kgx_sliced_counters.h) are plain integer C++ shared with
the kernel: tests/tools/sliced_counters_check.cpp, built with plain g++, drives them as by_genome_pass does -- pairs of
8-row blocks, the pending carry of an odd block, the flush every kBlocksPerFlush blocks -- against one add per bit: saturated
(all-ones) and dense random streams within and across flush periods, and the bound itself (one block pair more than the
planes hold does lose a carry)."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kgl_gene_amd" / "csrc"


def test_counters_header_is_host_only():
    text = (CSRC / "kgx_sliced_counters.h").read_text()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes and not [i for i in includes if "hip" in i or "kgx_" in i], includes
    # ... and it is the kernel's only definition of the structure
    kernels = (CSRC / "kgx_kernels_dosage.h").read_text()
    assert '#include "kgx_sliced_counters.h"' in kernels and "struct SlicedCounters" not in kernels


def test_counters_against_plain_counts(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/tools/sliced_counters_check.cpp")
    exe = tmp_path / "sliced_counters_check"
    subprocess.run([gxx, "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I", str(CSRC), "-o", str(exe),
                    str(ROOT / "tests" / "tools" / "sliced_counters_check.cpp")], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    print(res.stdout, res.stderr)
    assert res.returncode == 0, res.stderr
    assert " 0 failed" in res.stdout
