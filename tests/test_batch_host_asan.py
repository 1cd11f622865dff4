"""tests/cpp/batch_host_asan.cpp: the host-side passes over a batch — chain2aln's
checks and staging copy (bwa-flow_amd/csrc/batch_host.h), seeding's checks,
staging copy and gate table (seed_host.h) and the pass pool (host_pool.h) — as
a stand-alone program under AddressSanitizer and UBSan, then under
ThreadSanitizer, on the CPU."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_batch_host_passes_are_clean_under_the_sanitizers(tmp_path, sanitize):
    exe = str(tmp_path / "batch_host_asan")
    subprocess.run(["g++", "-std=c++17", "-g", f"-fsanitize={sanitize}", "-fno-sanitize-recover=all", "-pthread",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "bwa-flow_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "batch_host_asan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "batch_host_asan OK" in r.stdout, r.stdout + r.stderr
