"""The plan of a kgx_inbreed call (kgl_gene_amd/csrc/kgx_inbreed_plan.h) is host-only C++: tests/tools/inbreed_plan_check.cpp, built
with plain g++, walks it over a grid of shapes -- the segment cuts, the invariant that Loglikelihood on moments has a writer of
the hits' words, and which path each kind of call takes under the default switches and under the ones that change it."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kgl_gene_amd" / "csrc"


def test_plan_header_is_host_only():
    """No HIP runtime in the plan or in the constants it shares with the kernels."""
    for name in ("kgx_inbreed_plan.h", "kgx_inbreed_constants.h"):
        text = (CSRC / name).read_text()
        includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
        assert not [i for i in includes if "hip" in i], (name, includes)


def test_plan_over_the_grid(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/tools/inbreed_plan_check.cpp")
    exe = tmp_path / "inbreed_plan_check"
    subprocess.run([gxx, "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", "-I", str(CSRC), "-o", str(exe),
                    str(ROOT / "tests" / "tools" / "inbreed_plan_check.cpp")], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    print(res.stdout, res.stderr)
    assert res.returncode == 0, res.stderr
    assert " 0 failed" in res.stdout
