"""tests/cpp/xa_select_asan.cpp: xa_pri_idx and xa_over_cap (bwa-flow_amd/csrc/pure.h),
the per-region arithmetic of bwagpu_xa_select_device, as a stand-alone program
under AddressSanitizer and UBSan, on the CPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_xa_arithmetic_is_clean_and_is_the_references(tmp_path):
    exe = str(tmp_path / "xa_select_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "bwa-flow_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "xa_select_asan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "xa_select_asan OK" in r.stdout, r.stdout + r.stderr
