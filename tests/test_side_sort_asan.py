"""tests/cpp/side_sort_asan.cpp: the side lists' key prefix and short-run boundary
(bwa-flow_amd/csrc/side_sort.h) against a plain loop on random,
all-zero and one-key histograms, as a stand-alone program under
AddressSanitizer and UBSan, on the CPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
INC = ["-I", os.path.join(REPO, "bwa-flow_amd", "csrc")]


def test_prefix_and_short_boundary_match_a_plain_loop(tmp_path):
    exe = str(tmp_path / "side_sort_asan")
    subprocess.run(["g++", "-std=c++17", *SAN, *INC, os.path.join(REPO, "tests", "cpp", "side_sort_asan.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "side_sort_asan OK" in r.stdout, r.stdout + r.stderr
