"""Child process of tests/test_gpu_psd_project_many_large.py: one call of hipsdp_psd_project_many_large per mode on three jobs of
129 .. 200 rows, under whatever HIPSDP_PSD_LARGE_CHUNK the parent set.  Prints one JSON line: per mode the SHA-256 of every job's
(row, col, val) bytes, and how far the call moved the launch and read-back counters."""
import hashlib
import importlib.util
import json
import os
import sys

import psd_large_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def chunk_jobs():
    return [cases.random_job(160, 0.05, 0.5), cases.low_rank_shifted(200, 20, 0.25), cases.random_job(129, 1.0, 1e-4)]


def digest(res):
    h = hashlib.sha256()
    for a in res:
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    spec = importlib.util.spec_from_file_location("hipsdp_binding_child", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    hb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(hb)
    out = {}
    for mode in (0, 1):
        before = hb.psd_project_many_large_stats()
        res = hb.psd_project_many_large([j.args() for j in chunk_jobs()], cases.EPSILON, mode)
        after = hb.psd_project_many_large_stats()
        out["mode%d" % mode] = {"sha": [digest(r) for r in res], "calls": after[0] - before[0], "launches": after[1] - before[1],
                                "readbacks": after[2] - before[2]}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
