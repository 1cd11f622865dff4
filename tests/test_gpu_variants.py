"""The speculative path's A/B knobs,
each in a child process of its own (the library reads BWAGPU_* once per
process): round 5's emulation (no round-B task for an uncertain skip: the
final pass extends misses inline, round C runs for the long reads) and the
risky-first final pass.  Every variant must give the reference's regions, byte
for byte, on the C2 fixture's batches and the C5 fixture's mixed-length batch.
One child at a time.

The extension kernel of each form is ext_plan's alone (csrc/spec_plan.h): the
environment variables of the retired extension paths change nothing."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))

VARIANTS = {
    "emu_strict_off": {"BWAGPU_EMU_STRICT": "0"},
    "risky_first": {"BWAGPU_LIGHT_RISKY_FIRST": "1"},
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variant_parity(name):
    env = dict(os.environ, **VARIANTS[name])
    p = subprocess.run([sys.executable, os.path.join(HERE, "gpu_variant_child.py")], env=env, capture_output=True,
                       text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["c2"] and all(r["c2"]), r
    assert r["c5"] and all(r["c5"]), r


# the first length bin's kernel of forms 0, 1, 2 under the default scoring (ext_plan's table)
EXT_KERNELS_BY_FORM = ["spec_side4_kernel<16, 10, true>", "spec_ext2_kernel<5>", "spec_side4_kernel<32, 5, true>"]


def ext_kernels_of_child(extra_env):
    env = dict(os.environ, **extra_env)
    p = subprocess.run([sys.executable, os.path.join(HERE, "gpu_variant_child.py"), "ext_kernels"], env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])["ext_kernels"]


def test_ext_kernel_per_form_ignores_the_retired_knobs():
    """no kernel is launched: the plan's answer alone"""
    assert ext_kernels_of_child({}) == EXT_KERNELS_BY_FORM
    assert ext_kernels_of_child({"BWAGPU_EXT_PRODUCER": "1", "BWAGPU_EXT_PHASED": "0"}) == EXT_KERNELS_BY_FORM
