"""tests/cpp/r2_classify_asan.cpp: r2_classify (bwa-flow_amd/csrc/pure.h), the
per-job classifier of bwagpu_reg2aln_device, as a stand-alone program under
AddressSanitizer and UBSan, on the CPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_r2_classify_is_clean_and_keeps_the_band_inside_its_matrix(tmp_path):
    exe = str(tmp_path / "r2_classify_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "bwa-flow_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "r2_classify_asan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "r2_classify_asan OK" in r.stdout, r.stdout + r.stderr
