"""tests/cpp/rescue_host_asan.cpp: the host-side validation and span arithmetic of
bwagpu_pestat / bwagpu_mate_rescue (bwa-flow_amd/csrc/stage_host.h) as a
stand-alone program under AddressSanitizer and UBSan, on the CPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rescue_host_checks_are_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "rescue_host_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "bwa-flow_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "rescue_host_asan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "rescue_host_asan OK" in r.stdout, r.stdout + r.stderr
