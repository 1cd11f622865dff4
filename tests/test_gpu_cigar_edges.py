"""GPU parity of the CIGAR kernel at its band, segment and run-length
boundaries: the job families of tests/cigar_cases.py (what each reaches is
asserted on the CPU, tests/test_cigar_cases.py) against the reference's own
recorded outputs (tests/golden/cigar_edges.npz), one test per family.

bwagpu_reg2aln_batch must give the reference's record (every field), CIGAR op
and MD byte; bwagpu_reg2aln_device on the same jobs, with sentinel-filled
outputs, must give the host form's bytes and touch nothing outside the spans a
job writes.  The `capacity` family repeats both at every capacity of its list:
an overflowing job's status is ALN_OVERFLOW, its CIGAR and MD slots past what
the kernel may have begun stay as they were, and its neighbours' results do
not change."""
import numpy as np
import pytest

import cigar_cases as CC
import golden_io as G
from bwagpu import abi
from cigar_helpers import SENT, engine, run_device, same_as, untouched

pytestmark = pytest.mark.gpu

NAMES = list(CC.FAMILY_NAMES)   # the families themselves are built when a test first asks


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def refd():
    return G.load_ref()


@pytest.fixture(scope="module")
def gold():
    return G.load_cigar_edges()


def spans_untouched(out, cig, md):
    """past each job's n_cigar ops nothing of its CIGAR slot is written; past md_len + 1 bytes (the NUL)
    nothing of its MD slot; a job that is not ALN_OK has no CIGAR op written at all"""
    for k in range(len(out)):
        ok = out["status"][k] == abi.ALN_OK
        if not untouched(cig[k, int(out["n_cigar"][k]) if ok else 0:]):
            return f"job {k}: CIGAR slot written past its ops"
        if ok and not untouched(md[k, int(out["md_len"][k]) + 1:]):
            return f"job {k}: MD slot written past its NUL"
        if ok and md[k, int(out["md_len"][k])] != 0:
            return f"job {k}: MD not NUL-terminated"
    return None


@pytest.mark.parametrize("name", NAMES)
def test_family(torch, refd, gold, name):
    f, g = CC.families()[name], gold[name]
    assert np.array_equal(g["tasks"], f.tasks) and np.array_equal(g["qpool"], f.qpool), \
        "regenerate with oracle/gen_golden.py --only-cigar-edges"
    eng = engine(refd, f.opt)
    for c, (max_ops, max_md) in enumerate(f.calls):
        exp, ops, mds = g["calls"][c]
        out, cig, md = eng.reg2aln_batch(f.tasks, f.qpool, max_ops, max_md)
        bad = G.aln_mismatch(f.tasks, out, cig, md, exp, ops, mds)
        assert bad is None, f"{name} at ({max_ops}, {max_md}): {bad}; first differing job is {f.tags[int(bad.split('#')[1].split()[0])]}"
        assert out.tobytes() == exp.tobytes(), "a record byte outside the compared fields differs"
        dev = run_device(torch, eng, f.tasks, f.qpool, max_ops, max_md)
        assert same_as(f.tasks, dev, (out, cig, md)) is None, (max_ops, max_md)
        assert spans_untouched(*dev) is None, (max_ops, max_md)
        v = f.victims[c] if f.victims else None
        if v is not None:
            k, overflows, kind = v
            assert dev[0]["status"][k] == (abi.ALN_OVERFLOW if overflows else abi.ALN_OK), (f.tags[k], max_ops, max_md)
            if overflows and kind == "ops":   # refused before any op is written; the MD was complete
                assert untouched(dev[1][k])
            for n in (k - 1, k + 1):          # the neighbours' slots: what the reference recorded, nothing else
                if 0 <= n < len(f.tasks) and exp["status"][n] == abi.ALN_OK:
                    assert np.array_equal(dev[1][n, :exp["n_cigar"][n]], ops[n])
                    assert bytes(dev[2][n, :exp["md_len"][n]]) == mds[n] and dev[2][n, exp["md_len"][n]] == 0
                    assert (dev[2][n, int(exp["md_len"][n]) + 1:] == SENT).all()
    st = eng.last_stats()
    assert st["ext_calls"] >= len(f.tasks)
    eng.close()
