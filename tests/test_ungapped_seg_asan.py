"""tests/cpp/ungapped_seg_asan.cpp: the segment fold of the ungapped certificate's
scan (bwa-flow_amd/csrc/ungapped.h) against the serial scan on
random score sequences, as a stand-alone program under AddressSanitizer and
UBSan, on the CPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
INC = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "bwa-flow_amd", "csrc")]


def test_folds_match_the_serial_scan(tmp_path):
    exe = str(tmp_path / "ungapped_seg_asan")
    subprocess.run(["g++", "-std=c++17", *SAN, *INC, os.path.join(REPO, "tests", "cpp", "ungapped_seg_asan.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ungapped_seg_asan OK" in r.stdout, r.stdout + r.stderr
