"""Writes tests/golden/sdpi_signatures.json: the function declarations of SCIP-SDP's src/sdpi/sdpisolver.h (53) and
src/sdpi/lapack_interface.h (7), one line per function in the normal form gcc's -aux-info prints (types only, parameter
names dropped, SCIP's macro types such as SCIP_Real / SCIP_Bool expanded as SCIP's def.h expands them), read through the
test-only stand-ins of tests/scip_stubs/.  The tests compile the drop-in against these declarations
(tests/test_header_conformance.py) and build the host branch of the LAPACK interface with them
(tests/test_lapack_host_branch_cpu.py).  Data transcription; run once with the path of a SCIP-SDP source tree's src/
directory, output committed.

    python tests/golden/make_sdpi_signatures.py <SCIP-SDP>/src"""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
STUBS = os.path.join(os.path.dirname(HERE), "scip_stubs")
HEADERS = ("sdpi/sdpisolver.h", "sdpi/lapack_interface.h")


def main(src):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        tu = os.path.join(tmp, "decls.c")
        aux = os.path.join(tmp, "decls.aux")
        with open(tu, "w") as f:
            f.write("".join('#include "%s"\n' % h for h in HEADERS))
        subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-aux-info", aux, "-I" + STUBS, "-I" + src, tu], check=True)
        for h in HEADERS:
            path = os.path.join(os.path.abspath(src), h)
            decls = []
            for ln in open(aux):
                m = re.match(r"/\* (.*):\d+:N[CF] \*/ (.*;)", ln.strip())
                if m and os.path.abspath(m.group(1)) == path:
                    decls.append(m.group(2))
            out[h] = decls
    assert len(out["sdpi/sdpisolver.h"]) == 53 and len(out["sdpi/lapack_interface.h"]) == 7, {k: len(v) for k, v in out.items()}
    with open(os.path.join(HERE, "sdpi_signatures.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
