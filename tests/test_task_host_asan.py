"""tests/cpp/task_host_asan.cpp: the host-side plans of bwagpu_extend_batch,
bwagpu_align2_batch and bwagpu_sw_stream
(bwa-flow_amd/csrc/task_host.h) as a stand-alone program under
AddressSanitizer and UBSan, on the CPU."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_task_host_plans_are_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "task_host_asan")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "bwa-flow_amd", "csrc"),
                    os.path.join(REPO, "tests", "cpp", "task_host_asan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "task_host_asan OK" in r.stdout, r.stdout + r.stderr
