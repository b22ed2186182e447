"""The environment switches the engine and the solver interface read are exactly the ones INTEGRATION.md section 5 documents: a
switch added to the code needs a row in the table, and a switch retired from the code leaves the table with it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r"HIPSDP_[A-Z0-9_]+")


def _code_switches():
    # string literals, not getenv( calls: multi.hip hands HIPSDP_JOB_ID to its reader through an array of names
    found = set()
    for sub in ("csrc", "src"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, "scip-sdp_amd", sub)):
            for f in files:
                with open(os.path.join(dirpath, f), encoding="utf-8", errors="replace") as fh:
                    found.update(m[1:-1] for m in re.findall(r'"HIPSDP_[A-Z0-9_]+"', fh.read()))
    return found


def _documented_switches():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        text = fh.read()
    section = re.search(r"^## 5\..*?(?=^## )", text, re.S | re.M)
    assert section is not None, "INTEGRATION.md has no section 5"
    return set(NAME.findall(section.group(0)))


def test_documented_switches_match_the_code():
    code, doc = _code_switches(), _documented_switches()
    assert code, "no HIPSDP_* literal found under scip-sdp_amd/csrc and scip-sdp_amd/src"
    assert code - doc == set(), "read by the code but missing from INTEGRATION.md section 5"
    assert doc - code == set(), "documented in INTEGRATION.md section 5 but read nowhere"
