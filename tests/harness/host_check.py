"""host_check.py - TEST INFRASTRUCTURE.  The one place that knows how a host check program of tests/harness/*_check.cpp is built and
run: with the host compiler against the host-only sources of scip-sdp_amd/csrc, -fsanitize=address,undefined with the runtimes linked
in statically - a program of its own; nothing is loaded into python and nothing is preloaded."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "scip-sdp_amd", "csrc")


def run_clean(tmp_path, program, sources, ok_line):
    """compiles tests/harness/<program> with the files `sources` of scip-sdp_amd/csrc, runs it, and asserts a zero exit status, the
    line `ok_line` in its output and that neither sanitizer reported anything; returns the output"""
    exe = str(tmp_path / os.path.splitext(program)[0])
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + CSRC, os.path.join(ROOT, "tests", "harness", program)] + [os.path.join(CSRC, f) for f in sources] + ["-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and ok_line in r.stdout, r.stdout[-4000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error:" not in r.stdout, r.stdout[-4000:]
    return r.stdout
