"""ksw_extend2 task families at the edges of the range gates of the packed
16-bit extension (extend_quad, bwa-flow_amd/csrc/ksw_dev.h) and of the 32-bit
wave kernels.  Plain numpy, seeded, no GPU.  Every boundary number below comes
from the gate it names, never from a kernel's output:

  quad_bound_ok(o, hb)   pure.h   hb = h0 + qlen * max_mat for a bare task (task_host.h extend_plan)
      max_mat 1..15, every mat entry in [-127, 127]
      hb < 4096
      (hb << sk) + 128 < 32768, 2^sk > max_mat
      hb + 33 * 8 * e_ins < 32768
      o_del + 128 < 32768, oe_ins + 128 < 32768
  quad_rows_ok(o, tlen)  pure.h   tlen < 16384, (tlen + 256) * max(e_del, e_ins) < 28672
  wave_bound_ok(hb)      pure.h   hb < 2^21 (extend_plan refuses the batch otherwise)

A family is one option set and 40..150 tasks; side "in" holds the last value
the gate admits (bwagpu_extend_batch runs those tasks in the packed kernel;
tests/cpp/task_host_asan.cpp pins the routing), side "out" the first it
refuses (the tasks fall back to the wave kernels, or, for the 32-bit family,
the batch is refused).  Every family holds, per query length on the
columns-per-lane edges (QLENS):

  * a perfect match ending with the target, so that H climbs to exactly hb;
  * the same with target rows left over after the query's end;
  * one mismatch mid-query;
  * an insertion and a deletion of 1..3 bases a few columns before the end, so
    that E and F carry values next to the ceiling;
  * a peak some columns before the end and junk after it in query and target,
    so that the z-drop test runs from the ceiling.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from bwagpu import abi

QLENS = (1, 31, 32, 33, 63, 64, 127, 128, 255)


@dataclass
class Family:
    opt: dict
    tasks: np.ndarray
    qpool: np.ndarray
    tpool: np.ndarray
    gate: str        # the clause this family sits at
    side: str        # "in": the last admitted value, "out": the first refused one
    peak: int | None = None   # the largest H some task must reach exactly (the gate's hb), where the family claims one
    packed: bool = True       # "in" only: every task is one the packed kernel takes


def _opt(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, mat=None, w=100, zdrop=100):
    return dict(a=a, b=b, o_del=o_del, e_del=e_del, o_ins=o_ins, e_ins=e_ins, pen_clip5=5, pen_clip3=5, w=w,
                zdrop=zdrop, mat=abi.fill_scmat(a, b) if mat is None else np.asarray(mat, np.int8))


def max_mat(opt):
    return max(0, int(np.asarray(opt["mat"], np.int8).max()))  # ksw.c:397-398: from 0


class _Build:
    """tasks over one master target: target rows are master[:tlen]; queries are
    edited prefixes of the master"""

    def __init__(self, rng, master):
        self.rng, self.m = rng, np.asarray(master, np.uint8)
        self.tasks, self.qs, self.qo = [], [], 0

    def other(self, b):
        return (np.asarray(b, np.int64) + 1 + self.rng.integers(0, 3, np.shape(b))) % 4

    def add(self, q, tlen, h0, w=100, zdrop=100, eb=5):
        q = np.asarray(q, np.uint8)
        assert tlen <= len(self.m)
        self.tasks.append((self.qo, 0, len(q), tlen, w, eb, zdrop, h0))
        self.qs.append(q)
        self.qo += len(q)

    def variants(self, ql, h0, tail=40, tlen=None, **kw):
        """the six constructions of the module docstring for one query length;
        tlen: every task's target length (else the query's, plus `tail` rows)"""
        m, rng = self.m, self.rng
        t0 = ql if tlen is None else tlen
        t1 = ql + tail if tlen is None else tlen
        self.add(m[:ql], t0, h0, **kw)
        self.add(m[:ql], t1, h0, **kw)
        q = m[:ql].copy()
        q[ql // 2] = self.other(q[ql // 2])
        self.add(q, t1, h0, **kw)
        p, k = max(ql - 6, 0), int(rng.integers(1, 4))
        self.add(np.concatenate([m[:p], rng.integers(0, 4, k), m[p:]])[:ql], t1, h0, **kw)   # k extra query bases
        self.add(np.concatenate([m[:p], m[p + k:ql + k]]), t1, h0, **kw)                      # k target bases skipped
        if ql >= 63:
            p = ql - 40
            self.add(np.concatenate([m[:p], self.other(m[p:ql])]), t1, h0, **kw)

    def done(self, opt, gate, side, **kw):
        return Family(opt, np.array(self.tasks, abi.EXT_TASK_DTYPE), np.concatenate(self.qs).astype(np.uint8),
                      self.m.copy(), gate, side, **kw)


def _master(rng, n, base=None):
    """a random target; base: its first 258 bases (a query and an indel's worth) are that base, the rest never"""
    m = rng.integers(0, 4, n).astype(np.uint8)
    if base is not None:
        m[:258] = base
        m[258:] = (base + 1 + rng.integers(0, 3, n - 258)) % 4
    return m


def _score_family(rng, opt, hb, gate, side, peak, qlens=QLENS, base=None, packed=True):
    """every task's gate value h0 + qlen * max_mat is hb"""
    mm = max_mat(opt)
    b = _Build(rng, _master(rng, 400, base))
    qlens = [q for q in qlens if hb - q * mm >= 1]
    top = min(255, (hb - 1) // mm)
    if top not in qlens:
        qlens.append(top)  # the longest query whose h0 is still positive
    for ql in qlens:
        b.variants(ql, hb - ql * mm)
    return b.done(opt, gate, side, peak=peak, packed=packed)


def families(seed: int = 20260) -> dict:
    """-> {name: {"in": Family, "out": Family}} ("out" missing where a family has one side only)"""
    rng = np.random.default_rng(seed)
    fams: dict = {}

    def both(name, make):
        fams[name] = {"in": make("in"), "out": make("out")}

    # ---- score ceiling: quad_bound_ok's hb < 4096 binds for max_mat 1 and 3 (sk = 1, 2:
    # (hb << sk) + 128 < 32768 admits 16319 / 8159).  a=1, qlen 255: h0 3840 in, 3841 out.
    for a in (1, 3):
        both(f"ceiling_a{a}", lambda s, a=a: _score_family(
            rng, _opt(a=a), 4095 + (s == "out"), "quad_bound_ok: hb < 4096", s, 4095 + (s == "out")))
    # ---- shifted ceiling: (hb << sk) + 128 < 32768.  sk = 3 for max_mat 4..7: hb <= 4079;
    # sk = 4 for max_mat 8..15: hb <= 2039.  a=7, qlen 255: h0 2294 in.
    for a, top in ((4, 4079), (7, 4079), (8, 2039), (15, 2039)):
        both(f"shifted_a{a}", lambda s, a=a, top=top: _score_family(
            rng, _opt(a=a), top + (s == "out"), "quad_bound_ok: (hb << sk) + 128 < 32768", s, top + (s == "out")))
    # the only large entry is one diagonal cell: max_mat (and with it sk and hb) come from it
    # alone, and only a query of that base climbs by it
    diag = abi.fill_scmat(2, 4).copy()
    diag[0] = 15
    both("shifted_diag15", lambda s: _score_family(
        rng, _opt(a=2, b=4, mat=diag), 2039 + (s == "out"), "quad_bound_ok: (hb << sk) + 128 < 32768, max_mat from "
        "mat[0][0] alone", s, 2039 + (s == "out"), base=0))
    # a mismatch of -127 is the last matrix entry admitted, -128 the first refused (same hb, both admitted by it)
    both("mat_mismatch127", lambda s: _score_family(
        rng, _opt(a=4, b=127 + (s == "out")), 4079, "quad_bound_ok: mat entries in [-127, 127]", s, 4079))

    # ---- gap penalties: o_del + 128 < 32768 and oe_ins + 128 < 32768; hb = 4095 throughout.
    # SYM (extend_quad's o_del == o_ins form): o_del = o_ins = 32638 with e_ins = 1 is the
    # last pair oe_ins admits (o_del = 32639 would need e_ins = 0, which ksw_extend2's band
    # clamp divides by); one more is refused by oe_ins while o_del = 32639 alone is not.
    def gaps(s, **kw):
        return _score_family(rng, _opt(**kw), 4095, "quad_bound_ok: o_del + 128 < 32768, oe_ins + 128 < 32768", s, None)
    both("gap_o_del", lambda s: gaps(s, o_del=32639 + (s == "out")))
    both("gap_oe_ins", lambda s: gaps(s, o_ins=32638 + (s == "out"), e_ins=1))
    both("gap_sym", lambda s: gaps(s, o_del=32638 + (s == "out"), o_ins=32638 + (s == "out")))

    # ---- insertion scan: hb + 264 e_ins < 32768.  quad_rows_ok's (tlen + 256) max(e) < 28672
    # admits e_ins = 111 only for tlen <= 2 (258 * 111 = 28638, 259 * 111 = 28749), so these
    # tasks have one or two target rows: hb = 32767 - 264 * 111 = 3463 in, 3464 out.
    def ins_scan(s):
        opt, hb = _opt(o_ins=1, e_ins=111), 3463 + (s == "out")
        b = _Build(rng, _master(rng, 400))
        for ql in QLENS:
            for tl, mis in ((1, None), (2, None), (1, 0), (2, 1), (2, 0)):
                q = b.m[:ql].copy()
                if mis is not None and mis < ql:
                    q[mis] = b.other(q[mis])
                b.add(q, tl, hb - ql)
        return b.done(opt, "quad_bound_ok: hb + 33 * 8 * e_ins < 32768", s)
    both("ins_scan", ins_scan)

    # ---- rows: (tlen + 256) * max(e_del, e_ins) < 28672: 257 * 111 = 28527, 512 * 55 = 28160,
    # 1024 * 27 = 27648 in; e + 1 gives 28784, 28672, 28672 out.  hb = 3000 (+ 264 * 111 < 32768).
    for tl, e in ((1, 111), (256, 55), (768, 27)):
        def rows(s, tl=tl, e=e):
            e1 = e + (s == "out")
            b = _Build(rng, _master(rng, 800))
            for ql in QLENS:
                b.variants(ql, 3000 - ql, tlen=tl)
            return b.done(_opt(e_del=e1, e_ins=e1), "quad_rows_ok: (rows + 256) * max(e_del, e_ins) < 28672", s)
        both(f"rows_{tl}_{e}", rows)

    # tlen 16383 in, 16384 out, default band (a large w with a large end_bonus makes the
    # plan's LDS rows the refusal instead)
    def rows_tlen(s):
        b = _Build(rng, _master(rng, 16384))
        for ql in QLENS:
            b.variants(ql, 4095 - ql, tlen=16383 + (s == "out"))
        return b.done(_opt(), "quad_rows_ok: rows < 16384", s)
    both("rows_tlen", rows_tlen)

    # ---- z-drop clamp: extend_quad keeps min(zdrop, 32767) beside the 16-bit drop; H at the
    # ceiling, the peak 40 columns before the query's end
    def zclamp(s):
        b = _Build(rng, _master(rng, 400))
        for zd in (32766, 32767, 32768, 100000):
            for ql in (63, 64, 127, 128, 255):
                b.variants(ql, 4095 - ql, zdrop=zd)
        return b.done(_opt(), "extend_quad: ZD = min(zdrop, 32767)", s)
    fams["zdrop_clamp"] = {"in": zclamp("in")}

    # ---- the z-drop term |(i - max_i) - (j - max_j)| e: quad_rows_ok admits 28671, but the best
    # cell and every later row maximum lie on paths from h0, so the term stays near 2 hb.  This
    # family drives it as high as it goes: the best cell at the end of a perfect match, then a
    # long run of target rows kept alive by E alone (a deletion run of hb / e_del rows), and
    # the mirror with the peak mid-query; with the test off (zdrop 0) and at the clamp.  The
    # end bonus only widens ksw_extend2's band clamp (ksw.c:399-407), so that w decides.
    def zterm(s):
        b = _Build(rng, _master(rng, 700))
        for ql in (64, 128, 255):
            for zd in (0, 100000):
                for w in (100, 1000):
                    b.variants(ql, 4095 - ql, tail=400, w=w, zdrop=zd, eb=20000)
        return b.done(_opt(o_del=1, e_del=20, o_ins=1, e_ins=20), "quad_rows_ok: the z-drop term < 28672", s)
    fams["zdrop_term"] = {"in": zterm("in")}

    # ---- rows run: quad_rows_ok admits 16383, the plan's LDS rows about 4090 (task_host.h:
    # tb * 16 groups <= 64 KB).  a = 7 with a band of 1500: about 1750 rows.
    def long_rows(s):
        b = _Build(rng, _master(rng, 2400))
        for ql in QLENS:
            b.variants(ql, 4079 - 7 * ql, tlen=2400, w=1500, zdrop=0)
        return b.done(_opt(a=7), "quad_rows_ok: rows < 16384 (LDS rows bind first)", s)
    fams["rows_run"] = {"in": long_rows("in")}

    # ---- the 32-bit kernels: wave_bound_ok, hb < 2^21, at query lengths of each kExtVariants
    # list (qlen + 1 <= 192, 256, 1024).  The packed kernel takes none of these (hb >= 4096).
    def wave32(s):
        b = _Build(rng, _master(rng, 1200))
        hb = (1 << 21) - 1 + (s == "out")
        for ql in (100, 255, 700, 1022):
            for _ in range(2):
                b.variants(ql, hb - ql)
        return b.done(_opt(), "wave_bound_ok: hb < 2^21", s, peak=hb, packed=False)
    both("wave32", wave32)
    return fams


def flat(fams=None):
    """-> [(name, side, Family)] in a fixed order"""
    fams = families() if fams is None else fams
    return [(n, s, f) for n, d in fams.items() for s, f in d.items()]
