"""The stand-in headers the GPU packages build against here (kgx_refshim.h, kgx_pf7_resources.h) against the reference
headers they mirror: every public member function, enumerator and constant the shim declares must exist in the mirrored
reference class with the same signature.  scripts/check_refshim.py makes that comparison where a checkout of the reference
is at hand and records every shim declaration it verified in tests/golden/refshim_verified.json; this test needs nothing
outside the repository: it parses the shim with the same code and holds it, declaration for declaration, to that record.
A shim that declares anything else than what was verified fails here until the check has passed on it again."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_shim_declarations_match_the_reference_headers():
    sys.path.insert(0, str(ROOT / "scripts"))
    import check_refshim

    record = json.loads(check_refshim.RECORD.read_text())
    verified = record["verified"]
    assert len(verified) >= 100, len(verified)                   # the classes were found and parsed
    assert record["summary"].endswith(f"{len(verified)} identical in signature, 0 accepted differences, 0 problems"), record["summary"]
    rows = check_refshim.shim_declarations()
    was, now = {(c, n): a for c, n, a in verified}, {(c, n): a for c, n, a in rows}
    problems = [f"{c}::{n}: the shim declares {now.get((c, n))}, verified against the reference was {was.get((c, n))}"
                for c, n in sorted(set(was) | set(now)) if was.get((c, n)) != now.get((c, n))]
    assert not problems, "\n".join(problems)
    assert rows == verified                                      # the enumerators' order included
    # a member the packages lean on is really among the checked ones
    checked = {(c, n) for c, n, _ in rows}
    for needed in [("VirtualAnalysis", "fileReadAnalysis"), ("AnalysisResources", "getSingleResource"), ("HsGenomeGenealogyData", "getGenomeGenealogyRecord"),
                   ("InfoEvidenceAnalysis", "getTypedInfoData"), ("FrequencyDatabaseRead", "superPopFrequency"), ("GenomeDB", "getContig"),
                   ("Pf7SampleLocation", "sampleRadius"), ("Pf7FwsResource", "filterFWS")]:
        assert needed in checked, needed
