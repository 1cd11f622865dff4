"""tests/cpp/sam_text_asan.cpp: the decimal widths, the pa:f rounding and the flag,
TLEN and clip rules of bwagpu_sam_text_device (bwa-flow_amd/csrc/pure.h) as a
stand-alone program under AddressSanitizer and UBSan, on the CPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sam_text_arithmetic_is_clean_and_is_the_references(tmp_path):
    exe = str(tmp_path / "sam_text_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "bwa-flow_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "sam_text_asan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "sam_text_asan OK" in r.stdout, r.stdout + r.stderr
