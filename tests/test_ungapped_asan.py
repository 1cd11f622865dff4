"""tests/cpp/ungapped_asan.cpp: the ungapped certificate (bwa-flow_amd/csrc/ungapped.h)
against the project's own ksw_extend2 (oracle/ksw_ext.c) on random short calls,
as a stand-alone program under AddressSanitizer and UBSan, on the CPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
INC = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "oracle"),
       "-I", os.path.join(REPO, "bwa-flow_amd", "csrc")]


def test_certified_calls_match_ksw_extend2(tmp_path):
    obj, exe = str(tmp_path / "ksw_ext.o"), str(tmp_path / "ungapped_asan")
    subprocess.run(["gcc", *SAN, *INC, "-c", os.path.join(REPO, "oracle", "ksw_ext.c"), "-o", obj], check=True)
    subprocess.run(["g++", "-std=c++17", *SAN, *INC, os.path.join(REPO, "tests", "cpp", "ungapped_asan.cpp"), obj,
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ungapped_asan OK" in r.stdout, r.stdout + r.stderr
