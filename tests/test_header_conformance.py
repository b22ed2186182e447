"""The drop-in against the REFERENCE's own declarations: tests/golden/sdpi_signatures.json holds the 53 prototypes of SCIP-SDP's
src/sdpi/sdpisolver.h and the 7 of lapack_interface.h (written by tests/golden/make_sdpi_signatures.py).  scip-sdp_amd/src/sdpi/
sdpisolver_hip.c and lapack_interface_hip.c are compiled (syntax only) as the Makefile builds them, with those declarations forced in
after the stand-alone headers of include/: a definition or stand-alone prototype that disagrees with the reference prototype in any
argument is a hard compiler error ("conflicting types"), and every reference function must be defined by the drop-in."""
import json
import os
import re
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = os.path.join(ROOT, "tests", "golden", "sdpi_signatures.json")
CASES = {"sdpisolver_hip.c": ("sdpisolver_hip.h", "sdpi/sdpisolver.h"), "lapack_interface_hip.c": ("lapack_interface_hip.h", "sdpi/lapack_interface.h")}


@pytest.mark.parametrize("src", ["sdpisolver_hip.c", "lapack_interface_hip.c"])
def test_drop_in_compiles_against_the_reference_headers(src, tmp_path):
    own, ref = CASES[src]
    decls = json.load(open(SIGNATURES))[ref]
    forced = tmp_path / "reference_declarations.h"
    forced.write_text('#include "%s"\n%s\n' % (own, "\n".join(decls)))
    aux = tmp_path / "definitions.aux"
    cmd = ["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror=implicit-function-declaration", "-aux-info", str(aux),
           "-I" + os.path.join(ROOT, "scip-sdp_amd", "compat"), "-I" + os.path.join(ROOT, "include"), "-include", str(forced),
           os.path.join(ROOT, "scip-sdp_amd", "src", "sdpi", src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    assert "conflicting types" not in r.stdout and "warning" not in r.stdout, r.stdout
    defined = set(re.findall(r":NF \*/ [^(]*?(\w+) \(", aux.read_text()))
    names = [re.search(r"(\w+) \(", d).group(1) for d in decls]
    assert len(names) == {"sdpi/sdpisolver.h": 53, "sdpi/lapack_interface.h": 7}[ref]
    assert [x for x in names if x not in defined] == []
