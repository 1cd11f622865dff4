"""Python host mirror of the engine: flattened read batches and a per-device
Engine wrapping the C ABI.  Used by tests, smoke() and bench.py; the C++ host
(bwa-flow_amd/host/) uses the same ABI directly."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi


class BwaGpuError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{abi.ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


def _ptr(a: np.ndarray | None):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)


@dataclass
class Batch:
    """One ChainsRecord (src/Pipeline.h:46-57) in flattened form, see bwagpu_batch_t."""
    seq_off: np.ndarray         # int64 [n_reads+1]
    seq: np.ndarray             # uint8 nt4
    read_chain_off: np.ndarray  # int32 [n_reads+1]
    chain_seed_off: np.ndarray  # int32 [n_chains+1]
    chain_rid: np.ndarray       # int32 [n_chains]
    chain_frac_rep: np.ndarray  # float32 [n_chains]
    seeds: np.ndarray           # SEED_DTYPE [n_seeds]

    def __post_init__(self):
        self.seq_off = np.ascontiguousarray(self.seq_off, np.int64)
        self.seq = np.ascontiguousarray(self.seq, np.uint8)
        self.read_chain_off = np.ascontiguousarray(self.read_chain_off, np.int32)
        self.chain_seed_off = np.ascontiguousarray(self.chain_seed_off, np.int32)
        self.chain_rid = np.ascontiguousarray(self.chain_rid, np.int32)
        self.chain_frac_rep = np.ascontiguousarray(self.chain_frac_rep, np.float32)
        self.seeds = np.ascontiguousarray(self.seeds, abi.SEED_DTYPE)

    @property
    def n_reads(self) -> int:
        return len(self.seq_off) - 1

    @property
    def n_chains(self) -> int:
        return len(self.chain_seed_off) - 1

    @property
    def n_seeds(self) -> int:
        return len(self.seeds)

    def read_seed_off(self) -> np.ndarray:
        """first output slot of every read: chain_seed_off[read_chain_off[r]]"""
        return self.chain_seed_off[self.read_chain_off[:-1]]

    def to_c(self) -> abi.BatchC:
        b = abi.BatchC()
        b.n_reads, b.n_chains, b.n_seeds = self.n_reads, self.n_chains, self.n_seeds
        b.seq_bytes = int(self.seq_off[-1]) if self.n_reads >= 0 else 0
        b.seq_off = _ptr(self.seq_off)
        b.seq = _ptr(self.seq)
        b.read_chain_off = _ptr(self.read_chain_off)
        b.chain_seed_off = _ptr(self.chain_seed_off)
        b.chain_rid = _ptr(self.chain_rid)
        b.chain_frac_rep = _ptr(self.chain_frac_rep)
        b.seeds = _ptr(self.seeds)
        return b

    def subset(self, reads) -> "Batch":
        """a new batch holding the given reads (in the given order)"""
        reads = np.asarray(reads, np.int64)
        so, rco, cso = self.seq_off, self.read_chain_off, self.chain_seed_off
        seq_parts, seed_parts, rid, fr = [], [], [], []
        seq_off, rc_off, cs_off = [0], [0], [0]
        for r in reads:
            seq_parts.append(self.seq[so[r]:so[r + 1]])
            seq_off.append(seq_off[-1] + int(so[r + 1] - so[r]))
            for c in range(rco[r], rco[r + 1]):
                seed_parts.append(self.seeds[cso[c]:cso[c + 1]])
                cs_off.append(cs_off[-1] + int(cso[c + 1] - cso[c]))
                rid.append(self.chain_rid[c])
                fr.append(self.chain_frac_rep[c])
            rc_off.append(len(rid))
        return Batch(np.array(seq_off), np.concatenate(seq_parts) if seq_parts else np.zeros(0, np.uint8),
                     np.array(rc_off), np.array(cs_off), np.array(rid, np.int32), np.array(fr, np.float32),
                     np.concatenate(seed_parts) if seed_parts else np.zeros(0, abi.SEED_DTYPE))


def unflatten(batch: Batch, regs: np.ndarray, n: np.ndarray) -> list[np.ndarray]:
    """per-read region arrays (each the read's mem_alnreg_v contents in order)"""
    off = batch.read_seed_off()
    return [regs[off[r]:off[r] + n[r]] for r in range(batch.n_reads)]


def compact(batch: Batch, regs: np.ndarray, n: np.ndarray) -> np.ndarray:
    """concatenate the regions of all reads in read order"""
    n = np.asarray(n, np.int64)
    tot = int(n.sum())
    if tot == 0:
        return np.zeros(0, regs.dtype if regs is not None else abi.ALNREG_DTYPE)
    start = np.repeat(batch.read_seed_off().astype(np.int64), n)
    first = np.repeat(np.cumsum(n) - n, n)
    return regs[start + np.arange(tot, dtype=np.int64) - first]


class Engine:
    """One device context (bwagpu_create).  There is no CPU path behind it."""

    def __init__(self, device: int, opt: dict, l_pac: int, ann_offset, ann_len, pac=None,
                 pac_device_ptr: int | None = None):
        self.lib = abi.load()
        self.device = device
        self._args = (device, opt, l_pac, ann_offset, ann_len, pac, pac_device_ptr)
        self.opt = abi.opt_from_dict(opt)
        self._ann_off = np.ascontiguousarray(ann_offset, np.int64)
        self._ann_len = np.ascontiguousarray(ann_len, np.int32)
        self.bns = abi.Bns(int(l_pac), len(self._ann_off), 0, _ptr(self._ann_off), _ptr(self._ann_len))
        self.ctx = C.c_void_p()
        if pac_device_ptr is not None:
            rc = self.lib.bwagpu_create_resident(device, C.byref(self.opt), C.byref(self.bns),
                                                 C.c_void_p(pac_device_ptr), C.byref(self.ctx))
        else:
            self._pac = np.ascontiguousarray(pac, np.uint8)
            if len(self._pac) < int(l_pac) // 4 + 1:
                raise ValueError("pac shorter than l_pac/4+1 bytes")
            rc = self.lib.bwagpu_create(device, C.byref(self.opt), C.byref(self.bns), _ptr(self._pac),
                                        C.byref(self.ctx))
        if rc != abi.OK:
            raise BwaGpuError(rc, "bwagpu_create failed")

    def clone(self) -> "Engine":
        """another context on the same device with the same options and reference
        (a second stage worker); the FM-index is not carried over (set_bwt)"""
        return Engine(*self._args[:5], pac=self._args[5], pac_device_ptr=self._args[6])

    def close(self):
        if self.ctx:
            self.lib.bwagpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != abi.OK:
            raise BwaGpuError(rc, f"{what}: {self.lib.bwagpu_last_error(self.ctx).decode()}")

    def set_watchdog_ms(self, ms: int):
        self._check(self.lib.bwagpu_set_watchdog_ms(self.ctx, int(ms)), "set_watchdog_ms")

    def chain2aln(self, batch: Batch):
        """-> (regs[n_seeds] ALNREG_DTYPE, n[n_reads] int32)"""
        regs = np.zeros(max(batch.n_seeds, 1), abi.ALNREG_DTYPE)
        n = np.zeros(max(batch.n_reads, 1), np.int32)
        bc = batch.to_c()
        self._check(self.lib.bwagpu_chain2aln(self.ctx, C.byref(bc), _ptr(regs), _ptr(n)), "chain2aln")
        return regs[:batch.n_seeds], n[:batch.n_reads]

    def submit(self, slot: int, batch: Batch):
        bc = batch.to_c()
        self._check(self.lib.bwagpu_chain2aln_submit(self.ctx, slot, C.byref(bc)), "submit")

    def wait(self, slot: int, batch: Batch, out=None):
        """-> (regs, n) as chain2aln; `out` = (regs, n) arrays of at least
        max(n_seeds, 1) / max(n_reads, 1) entries to reuse instead of fresh ones"""
        if out is None:
            regs = np.zeros(max(batch.n_seeds, 1), abi.ALNREG_DTYPE)
            n = np.zeros(max(batch.n_reads, 1), np.int32)
        else:
            regs, n = out
            if (regs.dtype != abi.ALNREG_DTYPE or n.dtype != np.int32 or not regs.flags.c_contiguous
                    or not n.flags.c_contiguous or len(regs) < max(batch.n_seeds, 1) or len(n) < max(batch.n_reads, 1)):
                raise ValueError("wait: out arrays too small or of the wrong dtype/layout")
        self._check(self.lib.bwagpu_chain2aln_wait(self.ctx, slot, _ptr(regs), _ptr(n)), "wait")
        return regs[:batch.n_seeds], n[:batch.n_reads]

    def wait_dense(self, slot: int, batch: Batch, out=None):
        """-> (regs, n): the slot's results in read order without slot gaps
        (bwagpu_chain2aln_results_dense: only these regions crossed PCIe).
        out=None: numpy views onto the slot's pinned result buffers, valid
        until the slot's next submit (no host copy); `out` = (regs, n) arrays
        to copy into instead"""
        self._check(self.lib.bwagpu_chain2aln_wait(self.ctx, slot, None, None), "wait")
        rp, np_, op = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.bwagpu_chain2aln_results_dense(self.ctx, slot, C.byref(rp), C.byref(np_), C.byref(op)),
                    "results_dense")
        nr = batch.n_reads
        if nr == 0:
            return np.zeros(0, abi.ALNREG_DTYPE), np.zeros(0, np.int32)
        cnt = np.ctypeslib.as_array(C.cast(np_, C.POINTER(C.c_int32)), (nr,))
        tot = int(np.ctypeslib.as_array(C.cast(op, C.POINTER(C.c_int32)), (nr + 1,))[nr])
        view = (np.ctypeslib.as_array(C.cast(rp, C.POINTER(C.c_uint8)), (tot * abi.ALNREG_DTYPE.itemsize,))
                .view(abi.ALNREG_DTYPE) if tot else np.zeros(0, abi.ALNREG_DTYPE))
        if out is None:
            return view, cnt
        regs, n = out
        if len(regs) < tot or len(n) < nr:
            raise ValueError("wait_dense: out arrays too small")
        n[:nr] = cnt
        regs[:tot] = view
        return regs[:tot], n[:nr]

    def chain2aln_device(self, dev_batch: abi.BatchC, dev_out: int, dev_n: int, dev_stats: int | None,
                         stream: int | None):
        self._check(self.lib.bwagpu_chain2aln_device(self.ctx, C.byref(dev_batch), C.c_void_p(dev_out),
                                                     C.c_void_p(dev_n),
                                                     C.c_void_p(dev_stats) if dev_stats else None,
                                                     C.c_void_p(stream) if stream else None),
                    "chain2aln_device")

    def extend_batch(self, tasks: np.ndarray, qpool: np.ndarray, tpool: np.ndarray) -> np.ndarray:
        tasks = np.ascontiguousarray(tasks, abi.EXT_TASK_DTYPE)
        qpool = np.ascontiguousarray(qpool, np.uint8)
        tpool = np.ascontiguousarray(tpool, np.uint8)
        res = np.zeros(max(len(tasks), 1), abi.EXT_RES_DTYPE)
        self._check(self.lib.bwagpu_extend_batch(self.ctx, len(tasks), _ptr(tasks), _ptr(qpool), len(qpool),
                                                 _ptr(tpool), len(tpool), _ptr(res)), "extend_batch")
        return res[:len(tasks)]

    def align2_batch(self, tasks: np.ndarray, qpool: np.ndarray, tpool: np.ndarray) -> np.ndarray:
        """ksw_align2 (bwa/ksw.c:337-357) per task -> kswr_t records (abi.KSWR_DTYPE)"""
        tasks = np.ascontiguousarray(tasks, abi.ALIGN2_TASK_DTYPE)
        qpool = np.ascontiguousarray(qpool, np.uint8)
        tpool = np.ascontiguousarray(tpool, np.uint8)
        res = np.zeros(max(len(tasks), 1), abi.KSWR_DTYPE)
        self._check(self.lib.bwagpu_align2_batch(self.ctx, len(tasks), _ptr(tasks), _ptr(qpool), len(qpool),
                                                 _ptr(tpool), len(tpool), _ptr(res)), "align2_batch")
        return res[:len(tasks)]

    def align2_device(self, n: int, dev_tasks: int, dev_q: int, dev_t: int, dev_out: int, dev_scratch: int,
                      stream: int | None = None):
        """asynchronous launch on device buffers (pointers as ints, e.g. torch data_ptr())"""
        self._check(self.lib.bwagpu_align2_device(self.ctx, n, dev_tasks, dev_q, dev_t, dev_out, dev_scratch,
                                                  stream), "align2_device")

    def reg2aln_batch(self, tasks: np.ndarray, qpool: np.ndarray, max_ops: int = 64, max_md: int = 512):
        """mem_reg2aln's CIGAR part (bwa/bwamem.c:1104-1174) per job -> (abi.ALN_DTYPE records,
        CIGAR ops [n, max_ops] uint32, MD strings [n, max_md] bytes)"""
        tasks = np.ascontiguousarray(tasks, abi.REG2ALN_TASK_DTYPE)
        qpool = np.ascontiguousarray(qpool, np.uint8)
        n = len(tasks)
        out = np.zeros(max(n, 1), abi.ALN_DTYPE)
        cig = np.zeros((max(n, 1), max_ops), np.uint32)
        md = np.zeros((max(n, 1), max_md), np.uint8)
        self._check(self.lib.bwagpu_reg2aln_batch(self.ctx, n, _ptr(tasks), _ptr(qpool), len(qpool), max_ops, max_md,
                                                  _ptr(out), _ptr(cig), _ptr(md)), "reg2aln_batch")
        return out[:n], cig[:n], md[:n]

    def reg2aln_device(self, n_cap: int, dev_tasks: int, dev_qpool: int, qpool_len: int, dev_out: int,
                       dev_cigar: int, dev_md: int, max_ops: int = 64, max_md: int = 512,
                       dev_n_tasks: int | None = None, stream: int | None = None):
        """the same on device buffers (pointers as ints, e.g. torch data_ptr()), on stream: records at
        dev_out, job k's CIGAR at dev_cigar[k * max_ops], its MD at dev_md[k * max_md]; the job count is
        n_cap, or min(n_cap, *dev_n_tasks).  A job the kernel cannot take gets abi.ALN_REFUSED.  Waits for
        the stream once (the bin table); the bin kernels are left running and stream is ordered after them"""
        self._check(self.lib.bwagpu_reg2aln_device(
            self.ctx, int(n_cap), C.c_void_p(dev_n_tasks) if dev_n_tasks else None, C.c_void_p(dev_tasks),
            C.c_void_p(dev_qpool) if dev_qpool else None, int(qpool_len), int(max_ops), int(max_md),
            C.c_void_p(dev_out), C.c_void_p(dev_cigar), C.c_void_p(dev_md),
            C.c_void_p(stream) if stream else None), "reg2aln_device")

    def reg2aln_jobs_device(self, n_reads: int, dev_reg_off: int, dev_regs: int, dev_n: int, dev_select: int,
                            dev_seq_off: int, job_cap: int, dev_tasks: int, dev_job_of: int, dev_n_jobs: int,
                            stream: int | None = None):
        """the CIGAR jobs of the regions with dev_select >= 0 (pair_select_device's out_mapq fits), in
        (read, k) order, asynchronous on stream: dev_tasks[job_cap], dev_job_of parallel to the regions,
        dev_n_jobs = (written, needed); dev_n_jobs feeds reg2aln_device's dev_n_tasks"""
        self._check(self.lib.bwagpu_reg2aln_jobs_device(
            self.ctx, int(n_reads), C.c_void_p(dev_reg_off), C.c_void_p(dev_regs), C.c_void_p(dev_n),
            C.c_void_p(dev_select), C.c_void_p(dev_seq_off), int(job_cap),
            C.c_void_p(dev_tasks) if dev_tasks else None, C.c_void_p(dev_job_of), C.c_void_p(dev_n_jobs),
            C.c_void_p(stream) if stream else None), "reg2aln_jobs_device")

    def xa_select_device(self, n_reads: int, dev_reg_off: int, dev_regs: int, dev_n: int, dev_sel: int,
                         dev_out_mapq: int, dev_xa_of: int, dev_job_select: int, xopt: abi.SamOpt | None = None,
                         stream: int | None = None):
        """mem_gen_alt's selection on what pair_select_device left, asynchronous on stream: dev_xa_of (the
        region whose XA string a region joins, or -1) and dev_job_select (>= 0: the region needs a CIGAR),
        both parallel to the regions; dev_job_select feeds reg2aln_jobs_device's dev_select"""
        xo = abi.default_samopt() if xopt is None else xopt
        self._check(self.lib.bwagpu_xa_select_device(
            self.ctx, C.byref(xo), int(n_reads), C.c_void_p(dev_reg_off), C.c_void_p(dev_regs), C.c_void_p(dev_n),
            C.c_void_p(dev_sel), C.c_void_p(dev_out_mapq), C.c_void_p(dev_xa_of), C.c_void_p(dev_job_select),
            C.c_void_p(stream) if stream else None), "xa_select_device")

    def sam_text_device(self, t: abi.SamText, n_reads: int, stream: int | None = None, step: int | None = None):
        """the XA strings and mem_aln2sam on what the device chain left, asynchronous on stream: read r's SAM
        lines are dev_text[dev_text_off[r] : dev_text_off[r + 1]], dev_status per pair (abi.SAM_*),
        dev_text_n = (written, needed).  step (0 count, 1 scan, 2 write) runs that step alone, for timing"""
        st = C.c_void_p(stream) if stream else None
        if step is None:
            self._check(self.lib.bwagpu_sam_text_device(self.ctx, C.byref(t), int(n_reads), st), "sam_text_device")
        else:
            self._check(self.lib.bwagpu_debug_sam_text_step(self.ctx, C.byref(t), int(n_reads), int(step), st),
                        "debug_sam_text_step")

    def debug_reg2aln_times(self) -> dict:
        """the last reg2aln_device call (waits for it): the host's wait at the read-back, the bin kernels'
        span by HIP events, the host time of the call.  The first use only switches the timing on"""
        out = np.zeros(4, np.float64)
        self._check(self.lib.bwagpu_debug_reg2aln_times(self.ctx, _ptr(out)), "debug_reg2aln_times")
        return dict(wait_ms=float(out[0]), bins_ms=float(out[1]), call_ms=float(out[2]), jobs=int(out[3]))

    def set_bwt(self, hdr, words, sa=None, sa_intv: int = 32):
        """make the FM-index resident (hdr = primary, L2[0..4], seq_len as bwa's bwt_t;
        sa = the sampled suffix array, for bwt_sa)"""
        hdr = np.asarray(hdr, np.int64)
        self._bwt_words = np.ascontiguousarray(words, np.uint32)
        self._bwt_sa = None if sa is None else np.ascontiguousarray(sa, np.uint64)
        b = abi.BwtC()
        b.primary = int(hdr[0])
        for i in range(5):
            b.L2[i] = int(hdr[1 + i])
        b.seq_len = int(hdr[6])
        b.bwt_size = len(self._bwt_words)
        b.bwt = self._bwt_words.ctypes.data
        if self._bwt_sa is not None:
            b.sa_intv = sa_intv
            b.n_sa = len(self._bwt_sa)
            b.sa = self._bwt_sa.ctypes.data
        self._check(self.lib.bwagpu_set_bwt(self.ctx, C.byref(b)), "set_bwt")

    def bwt_sa(self, ks) -> np.ndarray:
        """bwt_sa (bwa/bwt.c:86-96) per BWT position"""
        ks = np.ascontiguousarray(ks, np.uint64)
        out = np.zeros(max(len(ks), 1), np.uint64)
        self._check(self.lib.bwagpu_bwt_sa(self.ctx, len(ks), _ptr(ks), _ptr(out)), "bwt_sa")
        return out[:len(ks)]

    def sw_stream(self, words: np.ndarray, cap_tasks: int) -> np.ndarray:
        """sw_top on the FPGA wire format (src/fpga/FPGAPipeline.cpp:252-336 in,
        :91-105 out): one packed task stream -> int16[n_tasks, 10] records"""
        words = np.ascontiguousarray(words, np.int32)
        out = np.zeros((max(cap_tasks, 1), 10), np.int16)
        n = C.c_int32(0)
        self._check(self.lib.bwagpu_sw_stream(self.ctx, _ptr(words), len(words), _ptr(out), int(cap_tasks),
                                              C.byref(n)), "sw_stream")
        return out[:n.value]

    # bwagpu_debug_ext_kernel codes (ext_plan, csrc/spec_plan.h) -> the first bin's extension kernel
    EXT_KERNELS = {2: "spec_ext2_kernel<5>",
                   # the phased pair: one "launch" = its left and right side launches
                   18: "spec_side4_kernel<16, 10, true>", 14: "spec_side4_kernel<32, 5, true>",
                   15: "spec_side4_kernel<32, 8, false>"}

    def ext_kernel(self, lq_max: int = 256) -> str:
        """the first length bin's extension kernel this context launches for
        reads of up to lq_max bases (the C side's own decision: ext_plan,
        csrc/spec_plan.h)"""
        k = self.lib.bwagpu_debug_ext_kernel(self.ctx, int(lq_max))
        if k not in self.EXT_KERNELS:
            raise BwaGpuError(k, "debug_ext_kernel")
        return self.EXT_KERNELS[k]

    def ext_form(self, form: int = -1) -> int:
        """this context's extension form (bwagpu_ctx_ext_form); -> the previous one"""
        return self.lib.bwagpu_ctx_ext_form(self.ctx, int(form))

    def ext_short(self, q: int = -1) -> int:
        """this context's short-side threshold (bwagpu_ctx_ext_short): sides with
        a query of 1 .. q bases run sixteen per wave in the eight-per-wave
        phased extension; 0 = off, -1 = query; -> the previous value"""
        return self.lib.bwagpu_ctx_ext_short(self.ctx, int(q))

    def ext_short_fill(self, percent: int = -1) -> int:
        """the smallest short run that takes the short phase, in percent of the
        launch's sixteen-per-wave call slots (bwagpu_ctx_ext_short_fill; 0 =
        every short run); -> the previous value"""
        return self.lib.bwagpu_ctx_ext_short_fill(self.ctx, int(percent))

    def light_pack(self, on: int = -1) -> int:
        """this context's packed light selection (bwagpu_ctx_light_pack): reads
        of up to eight seeds and chains eight per wave; 0 = one read per wave,
        -1 = query; -> the previous setting"""
        return self.lib.bwagpu_ctx_light_pack(self.ctx, int(on))

    def ungapped(self, on: int = -1) -> int:
        """this context's ungapped certificate (bwagpu_ctx_ungapped, default
        on; acts only while the row bound is on); -> the previous setting"""
        return self.lib.bwagpu_ctx_ungapped(self.ctx, int(on))

    def ungapped_right(self, on: int = -1) -> int:
        """this context's late settling of certified right sides behind a left
        side that needs the DP (bwagpu_ctx_ungapped_right, default on; acts
        only while the certificate does); -> the previous setting"""
        return self.lib.bwagpu_ctx_ungapped_right(self.ctx, int(on))

    def ungapped_right_counters(self, stream=None):
        """bwagpu_debug_spec_ungapped_right for the last device-entry batch on
        `stream` (a raw stream handle; None: the default stream) -> int64
        [3 rounds][settled after the left launch, their bases]"""
        out = np.zeros(6, np.int64)
        self._check(self.lib.bwagpu_debug_spec_ungapped_right(self.ctx, C.c_void_p(stream), _ptr(out)),
                    "debug_spec_ungapped_right")
        return out.reshape(3, 2)

    def fused_launches(self, mask: int = -1) -> int:
        """this context's fused launches (bwagpu_ctx_fused_launches, default 5):
        bit 1 the side lists' sort in two launches, bit 2 the late right sides
        beside the right launch, bit 4 heavy reads without a pair matrix in the
        scan's launch; 0 = every step a launch of its own; -> the previous mask"""
        return self.lib.bwagpu_ctx_fused_launches(self.ctx, int(mask))

    def emu_finish(self, on: int = -1) -> int:
        """this context's finishing of decided light reads in the emulate
        selection pass (bwagpu_ctx_emu_finish, default on); -> the previous setting"""
        return self.lib.bwagpu_ctx_emu_finish(self.ctx, int(on))

    def row_bound(self, on: int = -1) -> int:
        """this context's row bound in the packed extension kernels
        (bwagpu_ctx_row_bound, default on); -> the previous setting"""
        return self.lib.bwagpu_ctx_row_bound(self.ctx, int(on))

    def set_device_read_len(self, max_len: int):
        """bound on the read lengths of later device batches (bwagpu_set_device_read_len)"""
        self._check(self.lib.bwagpu_set_device_read_len(self.ctx, int(max_len)), "set_device_read_len")

    def sup_shift(self, shift: int):
        """superblock size 2^shift of the occurrence layout the NEXT set_bwt builds (tests; default 32)"""
        self._check(self.lib.bwagpu_debug_sup_shift(self.ctx, shift), "sup_shift")

    def seed_budget(self, budget: int):
        """bwt_extend calls a read gets on one lane before the wave kernel takes it (0: all on waves)"""
        self._check(self.lib.bwagpu_debug_seed_budget(self.ctx, budget), "seed_budget")

    def collect_intv(self, seq_off: np.ndarray, seq: np.ndarray, min_seed_len: int = 19, split_width: int = 10,
                     max_mem_intv: int = 20, split_factor: float = 1.5, max_per_read: int = 256,
                     out_cap: int | None = None, out: np.ndarray | None = None):
        """mem_collect_intv (bwa/bwamem.c:120-167) per read -> (counts int32[n], intervals INTV_DTYPE[sum]);
        out: the caller's INTV_DTYPE buffer to fill (reused across calls; its length is the capacity)"""
        seq_off = np.ascontiguousarray(seq_off, np.int64)
        seq = np.ascontiguousarray(seq, np.uint8)
        n = len(seq_off) - 1
        o = abi.SeedOpt(min_seed_len, split_width, max_mem_intv, split_factor)
        if out is not None:
            if out.dtype != abi.INTV_DTYPE or not out.flags.c_contiguous:
                raise ValueError("out must be a contiguous INTV_DTYPE array")
            cap = len(out)
        else:
            cap = max(n, 1) * max_per_read if out_cap is None else out_cap
            out = np.zeros(max(cap, 1), abi.INTV_DTYPE)
        cnt = np.zeros(max(n, 1), np.int32)
        self._check(self.lib.bwagpu_collect_intv(self.ctx, C.byref(o), n, _ptr(seq_off), _ptr(seq), max_per_read,
                                                 _ptr(out), cap, _ptr(cnt)), "collect_intv")
        cnt = cnt[:n]
        return cnt, out[:int(cnt.sum())]

    def set_alt(self, is_alt):
        """per-contig ALT flags for the chaining (None: none)"""
        self._alt = None if is_alt is None else np.ascontiguousarray(is_alt, np.uint8)
        self._check(self.lib.bwagpu_set_alt(self.ctx, None if self._alt is None else _ptr(self._alt)), "set_alt")

    @staticmethod
    def _seed_chain_opts(seedopt, split_factor, chainopt):
        so = np.asarray(seedopt, np.int32)
        co = abi.default_chainopt() if chainopt is None else chainopt
        return (abi.SeedOpt(int(so[0]), int(so[1]), int(so[2]), float(split_factor)),
                abi.ChainOpt(int(co["max_occ"]), int(co["max_chain_gap"]), int(co["min_chain_weight"]),
                             int(co["max_chain_extend"]), float(co["mask_level"]), float(co["drop_ratio"])))

    def seqs2chains(self, seq_off, seq, seedopt=(19, 10, 20), split_factor: float = 1.5, chainopt: dict | None = None,
                    raw: bool = False, copy: bool = True):
        """bwa-flow's SeqsToChains on the device (src/bwa_wrapper.cpp:105-115) ->
        (read_chain_off int32[n+1], chains CHAIN_DTYPE, chain_seed_off int32, seeds SEED_DTYPE);
        copy=False: views of the context's pinned output (valid until its next call)"""
        seq_off = np.ascontiguousarray(seq_off, np.int64)
        seq = np.ascontiguousarray(seq, np.uint8)
        n = len(seq_off) - 1
        so, co = self._seed_chain_opts(seedopt, split_factor, chainopt)
        out = abi.ChainsC()
        self._check(self.lib.bwagpu_seqs2chains(self.ctx, C.byref(so), C.byref(co), n, _ptr(seq_off), _ptr(seq),
                                                int(raw), C.byref(out)), "seqs2chains")
        nc, ns = out.n_chains, out.n_seeds

        def view(p, dt, k):
            if k == 0:
                return np.zeros(0, dt)
            v = np.frombuffer((C.c_char * (k * np.dtype(dt).itemsize)).from_address(p), dt)
            return v.copy() if copy else v
        return (view(out.read_chain_off, np.int32, n + 1), view(out.chains, abi.CHAIN_DTYPE, nc),
                view(out.chain_seed_off, np.int32, nc + 1), view(out.seeds, abi.SEED_DTYPE, ns))

    def seqs2regions(self, seq_off, seq, seedopt=(19, 10, 20), split_factor: float = 1.5,
                     chainopt: dict | None = None, copy: bool = True):
        """SeqsToChains + ChainsToRegions fused on the device -> (regions per read int32[n],
        regions ALNREG_DTYPE back to back in read order); copy=False: the regions as a
        view of the context's pinned output (valid until its next call)"""
        seq_off = np.ascontiguousarray(seq_off, np.int64)
        seq = np.ascontiguousarray(seq, np.uint8)
        n = len(seq_off) - 1
        so, co = self._seed_chain_opts(seedopt, split_factor, chainopt)
        cnt = np.zeros(max(n, 1), np.int32)
        regs, nreg = C.c_void_p(), C.c_int64()
        self._check(self.lib.bwagpu_seqs2regions(self.ctx, C.byref(so), C.byref(co), n, _ptr(seq_off), _ptr(seq),
                                                 _ptr(cnt), C.byref(regs), C.byref(nreg)), "seqs2regions")
        k = nreg.value
        out = np.zeros(0, abi.ALNREG_DTYPE) if k == 0 else np.frombuffer(
            (C.c_char * (k * abi.ALNREG_DTYPE.itemsize)).from_address(regs.value), abi.ALNREG_DTYPE)
        return cnt[:n], (out.copy() if copy else out)

    def regs_post(self, seq_off, seq, reg_off, regs, n, flags: int, id0: int = 0, popt: abi.PostOpt | None = None):
        """RegionsToSam::compute's per-read head (src/Pipeline.cpp:560-575) on the device:
        mem_sort_dedup_patch and the is_alt flag by flags (abi.POST_DEDUP_PATCH | abi.POST_MARK_ALT;
        abi.POST_PRIMARY is reserved and refused).
        Read r's n[r] regions at regs[reg_off[r]:] -> (regs, n) copies with the surviving
        regions at the front of every span"""
        seq_off = np.ascontiguousarray(seq_off, np.int64)
        seq = np.ascontiguousarray(seq, np.uint8)
        reg_off = np.ascontiguousarray(reg_off, np.int64)
        regs = np.array(regs, abi.ALNREG_DTYPE, order="C")
        n = np.array(n, np.int32, order="C")
        nr = len(seq_off) - 1
        if len(reg_off) < nr or len(n) < nr:
            raise ValueError("regs_post: reg_off / n shorter than the batch")
        po = abi.default_postopt() if popt is None else popt
        self._check(self.lib.bwagpu_regs_post(self.ctx, C.byref(po), int(flags), int(id0), nr, _ptr(seq_off),
                                              _ptr(seq), _ptr(reg_off), _ptr(regs), _ptr(n)), "regs_post")
        return regs, n

    def regs_post_device(self, dev_batch: abi.BatchC, dev_reg_off: int | None, dev_regs: int, dev_n: int,
                         flags: int, id0: int = 0, popt: abi.PostOpt | None = None, stream: int | None = None):
        """the same in place on device memory, asynchronous on stream (pointers as ints);
        dev_reg_off=None: the slot layout bwagpu_chain2aln_device writes"""
        po = abi.default_postopt() if popt is None else popt
        self._check(self.lib.bwagpu_regs_post_device(self.ctx, C.byref(po), int(flags), int(id0), C.byref(dev_batch),
                                                     C.c_void_p(dev_reg_off) if dev_reg_off else None,
                                                     C.c_void_p(dev_regs), C.c_void_p(dev_n),
                                                     C.c_void_p(stream) if stream else None), "regs_post_device")

    def set_regs_post(self, flags: int, id0: int = 0, popt: abi.PostOpt | None = None):
        """the switch (bwagpu_set_regs_post): flags != 0 makes chain2aln / submit+wait /
        seqs2regions return post-processed regions; id0 = the next batch's first read id"""
        po = abi.default_postopt() if popt is None else popt
        self._check(self.lib.bwagpu_set_regs_post(self.ctx, C.byref(po), int(flags), int(id0)), "set_regs_post")

    def pestat(self, reg_off, regs, n, popt: abi.PairOpt | None = None) -> np.ndarray:
        """mem_pestat (bwa/bwamem_pair.c:49-112) over a batch of interleaved pairs (reads 2i, 2i+1):
        read r's n[r] regions at regs[reg_off[r]:] -> pes[4] (abi.PESTAT_DTYPE), bit for bit the reference's"""
        reg_off = np.ascontiguousarray(reg_off, np.int64)
        regs = np.ascontiguousarray(regs, abi.ALNREG_DTYPE)
        n = np.ascontiguousarray(n, np.int32)
        if len(reg_off) != len(n):
            raise ValueError("pestat: reg_off and n differ in length")
        po = abi.default_pairopt() if popt is None else popt
        pes = np.zeros(4, abi.PESTAT_DTYPE)
        self._check(self.lib.bwagpu_pestat(self.ctx, C.byref(po), len(n), _ptr(reg_off), _ptr(regs), _ptr(n),
                                           _ptr(pes)), "pestat")
        return pes

    def pestat_device(self, n_reads: int, dev_reg_off: int, dev_regs: int, dev_n: int, dev_pes: int,
                      popt: abi.PairOpt | None = None, stream: int | None = None):
        """the same on device memory, asynchronous on stream (pointers as ints); dev_pes: 4 x 32 bytes"""
        po = abi.default_pairopt() if popt is None else popt
        self._check(self.lib.bwagpu_pestat_device(self.ctx, C.byref(po), int(n_reads), C.c_void_p(dev_reg_off),
                                                  C.c_void_p(dev_regs), C.c_void_p(dev_n), C.c_void_p(dev_pes),
                                                  C.c_void_p(stream) if stream else None), "pestat_device")

    def mate_rescue(self, pes, seq_off, seq, reg_off, regs, n, out_off, popt: abi.PairOpt | None = None):
        """the rescue loop of mem_sam_pe (bwa/bwamem_pair.c:268-279, mem_matesw) for every pair of a batch.
        Read r's result may hold out_off[r+1] - out_off[r] regions ->
        (out_regs[out_off[-1]], out_n[n_reads], status[n_reads/2] abi.RESCUE_*, n_sw[n_reads/2])"""
        pes = np.ascontiguousarray(pes, abi.PESTAT_DTYPE)
        seq_off = np.ascontiguousarray(seq_off, np.int64)
        seq = np.ascontiguousarray(seq, np.uint8)
        reg_off = np.ascontiguousarray(reg_off, np.int64)
        regs = np.ascontiguousarray(regs, abi.ALNREG_DTYPE)
        n = np.ascontiguousarray(n, np.int32)
        out_off = np.ascontiguousarray(out_off, np.int64)
        nr = len(seq_off) - 1
        if len(pes) != 4 or len(reg_off) < nr or len(n) < nr or len(out_off) != nr + 1:
            raise ValueError("mate_rescue: pes / reg_off / n / out_off do not fit the batch")
        po = abi.default_pairopt() if popt is None else popt
        out = np.zeros(max(int(out_off[-1]), 1), abi.ALNREG_DTYPE)
        out_n = np.zeros(max(nr, 1), np.int32)
        status = np.zeros(max(nr // 2, 1), np.int32)
        n_sw = np.zeros(max(nr // 2, 1), np.int32)
        self._check(self.lib.bwagpu_mate_rescue(self.ctx, C.byref(po), _ptr(pes), nr, _ptr(seq_off), _ptr(seq),
                                                _ptr(reg_off), _ptr(regs), _ptr(n), _ptr(out_off), _ptr(out),
                                                _ptr(out_n), _ptr(status), _ptr(n_sw)), "mate_rescue")
        return out, out_n[:nr], status[:nr // 2], n_sw[:nr // 2]

    def mate_rescue_device(self, dev_pes: int, dev_batch: abi.BatchC, dev_reg_off: int, dev_regs: int, dev_n: int,
                           dev_out_off: int, dev_out_regs: int, dev_out_n: int, dev_status: int, dev_n_sw: int,
                           popt: abi.PairOpt | None = None, stream: int | None = None):
        """the same on device memory, on stream (pointers as ints): directly after regs_post_device /
        pestat_device on that stream; dev_batch needs n_reads, seq_bytes, seq_off, seq"""
        po = abi.default_pairopt() if popt is None else popt
        self._check(self.lib.bwagpu_mate_rescue_device(
            self.ctx, C.byref(po), C.c_void_p(dev_pes), C.byref(dev_batch), C.c_void_p(dev_reg_off),
            C.c_void_p(dev_regs), C.c_void_p(dev_n), C.c_void_p(dev_out_off), C.c_void_p(dev_out_regs),
            C.c_void_p(dev_out_n), C.c_void_p(dev_status), C.c_void_p(dev_n_sw),
            C.c_void_p(stream) if stream else None), "mate_rescue_device")

    def mark_primary(self, reg_off, regs, n, id0: int = 0, sopt: abi.SelOpt | None = None):
        """mem_mark_primary_se (bwa/bwamem.c:502-567) for every read of a batch, read r with id0 + r:
        read r's n[r] regions at regs[reg_off[r]:] -> (regs copy reordered and marked, n_pri[n_reads],
        status[n_reads] abi.SEL_*)"""
        reg_off = np.ascontiguousarray(reg_off, np.int64)
        regs = np.array(regs, abi.ALNREG_DTYPE, order="C")
        n = np.ascontiguousarray(n, np.int32)
        if len(reg_off) != len(n):
            raise ValueError("mark_primary: reg_off and n differ in length")
        so = abi.default_selopt() if sopt is None else sopt
        nr = len(n)
        n_pri = np.zeros(max(nr, 1), np.int32)
        status = np.zeros(max(nr, 1), np.int32)
        self._check(self.lib.bwagpu_mark_primary(self.ctx, C.byref(so), int(id0), nr, _ptr(reg_off), _ptr(regs),
                                                 _ptr(n), _ptr(n_pri), _ptr(status)), "mark_primary")
        return regs, n_pri[:nr], status[:nr]

    def mark_primary_device(self, n_reads: int, dev_reg_off: int, dev_regs: int, dev_n: int, dev_n_pri: int,
                            dev_status: int, id0: int = 0, sopt: abi.SelOpt | None = None,
                            stream: int | None = None):
        """the same in place on device memory, asynchronous on stream (pointers as ints)"""
        so = abi.default_selopt() if sopt is None else sopt
        self._check(self.lib.bwagpu_mark_primary_device(
            self.ctx, C.byref(so), int(id0), int(n_reads), C.c_void_p(dev_reg_off), C.c_void_p(dev_regs),
            C.c_void_p(dev_n), C.c_void_p(dev_n_pri), C.c_void_p(dev_status),
            C.c_void_p(stream) if stream else None), "mark_primary_device")

    def pair_select(self, pes, reg_off, regs, n, n_pri, pair_id0: int = 0, sopt: abi.SelOpt | None = None,
                    in_status=None):
        """mem_sam_pe from bwa/bwamem_pair.c:286 to its first mem_reg2aln for every pair (reads 2i, 2i+1;
        pair i has id pair_id0 + i) on regions as mark_primary leaves them ->
        (sel[n_reads/2] abi.PAIRSEL_DTYPE, out_mapq parallel to regs (-1: no record), regs copy as the
        reference leaves them)"""
        pes = np.ascontiguousarray(pes, abi.PESTAT_DTYPE)
        reg_off = np.ascontiguousarray(reg_off, np.int64)
        regs = np.array(regs, abi.ALNREG_DTYPE, order="C")
        n = np.ascontiguousarray(n, np.int32)
        n_pri = np.ascontiguousarray(n_pri, np.int32)
        if len(pes) != 4 or len(reg_off) != len(n) or len(n_pri) != len(n):
            raise ValueError("pair_select: pes / reg_off / n / n_pri do not fit the batch")
        nr = len(n)
        if in_status is not None:
            in_status = np.ascontiguousarray(in_status, np.int32)
            if len(in_status) != nr // 2:
                raise ValueError("pair_select: in_status is not one word per pair")
        so = abi.default_selopt() if sopt is None else sopt
        sel = np.zeros(max(nr // 2, 1), abi.PAIRSEL_DTYPE)
        out_mapq = np.full(max(len(regs), 1), -1, np.int32)
        self._check(self.lib.bwagpu_pair_select(self.ctx, C.byref(so), _ptr(pes), int(pair_id0), nr, _ptr(reg_off),
                                                _ptr(regs), _ptr(n), _ptr(n_pri), _ptr(in_status), _ptr(sel),
                                                _ptr(out_mapq)), "pair_select")
        return sel[:nr // 2], out_mapq[:len(regs)], regs

    def pair_select_device(self, dev_pes: int, n_reads: int, dev_reg_off: int, dev_regs: int, dev_n: int,
                           dev_n_pri: int, dev_in_status: int | None, dev_sel: int, dev_out_mapq: int,
                           pair_id0: int = 0, sopt: abi.SelOpt | None = None, stream: int | None = None):
        """the same on device memory, on stream (pointers as ints): directly after mark_primary_device"""
        so = abi.default_selopt() if sopt is None else sopt
        self._check(self.lib.bwagpu_pair_select_device(
            self.ctx, C.byref(so), C.c_void_p(dev_pes), int(pair_id0), int(n_reads), C.c_void_p(dev_reg_off),
            C.c_void_p(dev_regs), C.c_void_p(dev_n), C.c_void_p(dev_n_pri),
            C.c_void_p(dev_in_status) if dev_in_status else None, C.c_void_p(dev_sel), C.c_void_p(dev_out_mapq),
            C.c_void_p(stream) if stream else None), "pair_select_device")

    def debug_rescue_drop(self, k: int):
        """tests: the first round's plan of later mate_rescue calls leaves every k-th task out (0 = off)"""
        self._check(self.lib.bwagpu_debug_rescue_drop(self.ctx, int(k)), "debug_rescue_drop")

    @staticmethod
    def debug_live_buffers() -> tuple[int, int]:
        """-> (buffers, bytes) that all contexts of this process hold at the moment"""
        n, b = C.c_int64(), C.c_int64()
        rc = abi.load().bwagpu_debug_live_buffers(C.byref(n), C.byref(b))
        if rc != abi.OK:
            raise BwaGpuError(rc, "debug_live_buffers")
        return n.value, b.value

    def debug_rescue_times(self) -> dict:
        """the last mate_rescue* call by HIP events, summed over its rounds (waits for it)"""
        out = np.zeros(4, np.float64)
        self._check(self.lib.bwagpu_debug_rescue_times(self.ctx, _ptr(out)), "debug_rescue_times")
        return dict(plan_ms=float(out[0]), align2_ms=float(out[1]), apply_ms=float(out[2]), rounds=int(out[3]))

    def prof_start(self, max_launches: int):
        """time the next max_launches launches of the dominant extension kernel"""
        self._check(self.lib.bwagpu_prof_start(self.ctx, max_launches), "prof_start")

    def prof_intervals(self, max_n: int = 4096):
        """-> float64[n, 2]: each timed launch's [start, end] in ms from the first event"""
        a = np.zeros(max(max_n, 1), np.float64)
        b = np.zeros(max(max_n, 1), np.float64)
        n = C.c_int32(0)
        self._check(self.lib.bwagpu_prof_intervals(self.ctx, _ptr(a), _ptr(b), int(max_n), C.byref(n)), "prof_intervals")
        return np.stack([a[:n.value], b[:n.value]], axis=1)

    def prof_read(self) -> tuple[float, int]:
        """-> (summed kernel ms, launches timed) since prof_start"""
        ms, n = C.c_double(), C.c_int32()
        self._check(self.lib.bwagpu_prof_read(self.ctx, C.byref(ms), C.byref(n)), "prof_read")
        return ms.value, n.value

    def last_stats(self, slot: int = 0) -> dict:
        s = abi.Stats()
        self._check(self.lib.bwagpu_last_stats(self.ctx, slot, C.byref(s)), "last_stats")
        return {k: getattr(s, k) for k, _ in abi.Stats._fields_}
