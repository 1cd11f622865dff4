"""tests/cpp/ext_plan_asan.cpp: ext_plan (bwa-flow_amd/csrc/spec_plan.h), the
choice of extension kernel per length bin, against a transcription of the
launch code it replaced, as a stand-alone program under AddressSanitizer and
UBSan, on the CPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ext_plan_matches_the_launch_code_it_replaced(tmp_path):
    exe = str(tmp_path / "ext_plan_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "bwa-flow_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "ext_plan_asan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "ext_plan_asan OK" in r.stdout, r.stdout + r.stderr
