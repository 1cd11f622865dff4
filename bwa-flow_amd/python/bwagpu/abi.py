"""ctypes mirror of include/bwagpu.h (the engine's C ABI) + numpy record dtypes.

The record dtypes are byte-for-byte the reference's structs:
  SEED_DTYPE   == mem_seed_t   (src/bwa_wrapper.h:62-66, 24 B)
  ALNREG_DTYPE == mem_alnreg_t (bwa/bwamem.h:60-79, 88 B)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_ROOT = os.path.normpath(os.path.join(HERE, "..", ".."))  # bwa-flow_amd/
REPO_ROOT = os.path.normpath(os.path.join(PKG_ROOT, ".."))
LIB_DIR = os.path.join(PKG_ROOT, "lib")

ABI_VERSION = 1
OK, E_INVAL, E_NOMEM, E_DEVICE, E_HANG, E_RESULTS, E_UNSUPPORTED, E_NODEVICE = range(8)
ERR_NAMES = {
    OK: "OK", E_INVAL: "E_INVAL", E_NOMEM: "E_NOMEM", E_DEVICE: "E_DEVICE", E_HANG: "E_HANG",
    E_RESULTS: "E_RESULTS", E_UNSUPPORTED: "E_UNSUPPORTED", E_NODEVICE: "E_NODEVICE",
}
MAX_READ_LEN = 1023
NUM_SLOTS = 4

SEED_DTYPE = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4"), ("score", "<i4"),
                       ("pad", "<i4")])
ALNREG_DTYPE = np.dtype([
    ("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("rid", "<i4"), ("score", "<i4"),
    ("truesc", "<i4"), ("sub", "<i4"), ("alt_sc", "<i4"), ("csub", "<i4"), ("sub_n", "<i4"),
    ("w", "<i4"), ("seedcov", "<i4"), ("secondary", "<i4"), ("secondary_all", "<i4"),
    ("seedlen0", "<i4"), ("n_comp_is_alt", "<u4"), ("frac_rep", "<f4"), ("hash", "<u8")])
EXT_TASK_DTYPE = np.dtype([("qoff", "<i8"), ("toff", "<i8"), ("qlen", "<i4"), ("tlen", "<i4"),
                           ("w", "<i4"), ("end_bonus", "<i4"), ("zdrop", "<i4"), ("h0", "<i4")])
EXT_RES_DTYPE = np.dtype([("score", "<i4"), ("qle", "<i4"), ("tle", "<i4"), ("gtle", "<i4"),
                          ("gscore", "<i4"), ("max_off", "<i4")])
ALIGN2_TASK_DTYPE = np.dtype([("qoff", "<i8"), ("toff", "<i8"), ("qlen", "<i4"), ("tlen", "<i4"),
                              ("xtra", "<i4"), ("pad", "<i4")])
KSWR_DTYPE = np.dtype([("score", "<i4"), ("te", "<i4"), ("qe", "<i4"), ("score2", "<i4"), ("te2", "<i4"),
                       ("tb", "<i4"), ("qb", "<i4")])
KSW_XBYTE, KSW_XSTOP, KSW_XSUBO, KSW_XSTART = 0x10000, 0x20000, 0x40000, 0x80000
REG2ALN_TASK_DTYPE = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qoff", "<i8"), ("l_seq", "<i4"), ("qb", "<i4"),
                               ("qe", "<i4"), ("truesc", "<i4"), ("w", "<i4"), ("pad", "<i4")])
ALN_DTYPE = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("is_rev", "<i4"), ("n_cigar", "<i4"), ("NM", "<i4"),
                      ("md_len", "<i4"), ("score", "<i4"), ("w", "<i4"), ("status", "<i4")])
ALN_OK, ALN_NO_CIGAR, ALN_OVERFLOW, ALN_UNMAPPED, ALN_REFUSED = 0, 1, 2, 3, 4
assert REG2ALN_TASK_DTYPE.itemsize == 48 and ALN_DTYPE.itemsize == 40
assert SEED_DTYPE.itemsize == 24 and ALNREG_DTYPE.itemsize == 88
assert ALIGN2_TASK_DTYPE.itemsize == 32 and KSWR_DTYPE.itemsize == 28
assert EXT_TASK_DTYPE.itemsize == 40 and EXT_RES_DTYPE.itemsize == 24


class Opt(C.Structure):
    """bwagpu_opt_t: the mem_opt_t fields (bwa/bwamem.h:26-58) the path reads."""
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("o_del", C.c_int32), ("e_del", C.c_int32),
                ("o_ins", C.c_int32), ("e_ins", C.c_int32), ("pen_clip5", C.c_int32),
                ("pen_clip3", C.c_int32), ("w", C.c_int32), ("zdrop", C.c_int32),
                ("mat", C.c_int8 * 25), ("pad_", C.c_int8 * 3)]


class Bns(C.Structure):
    _fields_ = [("l_pac", C.c_int64), ("n_seqs", C.c_int32), ("pad_", C.c_int32),
                ("ann_offset", C.c_void_p), ("ann_len", C.c_void_p)]


class BatchC(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("n_chains", C.c_int32), ("n_seeds", C.c_int32),
                ("pad_", C.c_int32), ("seq_bytes", C.c_int64), ("seq_off", C.c_void_p),
                ("seq", C.c_void_p), ("read_chain_off", C.c_void_p), ("chain_seed_off", C.c_void_p),
                ("chain_rid", C.c_void_p), ("chain_frac_rep", C.c_void_p), ("seeds", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("total_ms", C.c_double), ("cells", C.c_int64),
                ("rows", C.c_int64), ("ext_calls", C.c_int64), ("h2d_bytes", C.c_int64),
                ("d2h_bytes", C.c_int64)]


class BwtC(C.Structure):
    """bwagpu_bwt_t == bwt_t's header + occurrence words (bwa/bwt.h:46-57)"""
    _fields_ = [("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("seq_len", C.c_uint64),
                ("bwt_size", C.c_uint64), ("bwt", C.c_void_p), ("sa_intv", C.c_int32), ("pad_", C.c_int32),
                ("n_sa", C.c_uint64), ("sa", C.c_void_p)]


class SeedOpt(C.Structure):
    """bwagpu_seedopt_t: mem_opt_t's seeding fields (bwamem.c:62-72)"""
    _fields_ = [("min_seed_len", C.c_int32), ("split_width", C.c_int32), ("max_mem_intv", C.c_int32),
                ("split_factor", C.c_float)]


INTV_DTYPE = np.dtype([("x", "<u8", (3,)), ("info", "<u8")])  # bwagpu_intv_t == bwtintv_t
assert INTV_DTYPE.itemsize == 32

# bwagpu_chain_t: mem_chain_t (bwa/bwamem.c:180-186) without its seed vector
CHAIN_DTYPE = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("n", "<i4"), ("w", "<i4"), ("kept", "<i4"),
                        ("first", "<i4"), ("is_alt", "<i4"), ("frac_rep", "<f4"), ("pad_", "<i4")])
assert CHAIN_DTYPE.itemsize == 40


class ChainOpt(C.Structure):
    """bwagpu_chainopt_t: mem_opt_t's chaining fields (bwamem.c:62-72)"""
    _fields_ = [("max_occ", C.c_int32), ("max_chain_gap", C.c_int32), ("min_chain_weight", C.c_int32),
                ("max_chain_extend", C.c_int32), ("mask_level", C.c_float), ("drop_ratio", C.c_float)]


class ChainsC(C.Structure):
    """bwagpu_chains_t: a batch's chains in the bwagpu_batch_t layout"""
    _fields_ = [("n_reads", C.c_int32), ("n_chains", C.c_int32), ("n_seeds", C.c_int64),
                ("read_chain_off", C.c_void_p), ("chain_seed_off", C.c_void_p), ("chains", C.c_void_p),
                ("seeds", C.c_void_p)]


class PostOpt(C.Structure):
    """bwagpu_postopt_t: mem_opt_t's fields of mem_sort_dedup_patch / mem_mark_primary_se"""
    _fields_ = [("max_chain_gap", C.c_int32), ("mask_level_redun", C.c_float), ("mask_level", C.c_float),
                ("pad_", C.c_int32)]


POST_DEDUP_PATCH, POST_MARK_ALT, POST_PRIMARY = 1, 2, 4


def default_postopt() -> PostOpt:
    """mem_opt_init's defaults (bwa/bwamem.c:62-72)"""
    return PostOpt(10000, 0.95, 0.50, 0)


class PairOpt(C.Structure):
    """bwagpu_pairopt_t: mem_opt_t's fields of mem_pestat / mem_matesw, and the round cap of mate rescue"""
    _fields_ = [("max_ins", C.c_int32), ("max_matesw", C.c_int32), ("pen_unpaired", C.c_int32),
                ("min_seed_len", C.c_int32), ("max_chain_gap", C.c_int32), ("mask_level_redun", C.c_float),
                ("mask_level", C.c_float), ("max_rounds", C.c_int32)]


def default_pairopt() -> PairOpt:
    """mem_opt_init's defaults (bwa/bwamem.c:48-84); three rounds"""
    return PairOpt(10000, 50, 17, 19, 10000, 0.95, 0.50, 3)


# bwagpu_pestat_t == mem_pestat_t (bwa/bwamem.h:82-86)
PESTAT_DTYPE = np.dtype([("low", "<i4"), ("high", "<i4"), ("failed", "<i4"), ("pad", "<i4"), ("avg", "<f8"),
                         ("std", "<f8")])
assert PESTAT_DTYPE.itemsize == 32 and C.sizeof(PairOpt) == 32
RESCUE_DONE, RESCUE_UNFINISHED, RESCUE_OVERFLOW, RESCUE_UNSUPPORTED = 0, 1, 2, 3


class SelOpt(C.Structure):
    """bwagpu_selopt_t: mem_opt_t's fields of mem_mark_primary_se, mem_pair's caller and mem_approx_mapq_se"""
    _fields_ = [("T", C.c_int32), ("pen_unpaired", C.c_int32), ("min_seed_len", C.c_int32),
                ("mapQ_coef_len", C.c_float), ("mapQ_coef_fac", C.c_int32), ("mask_level", C.c_float),
                ("drop_ratio", C.c_float), ("flags", C.c_int32)]


def default_selopt(flags: int = 0) -> SelOpt:
    """mem_opt_init's defaults (bwa/bwamem.c:48-84): mapQ_coef_fac is (int)log(50)"""
    return SelOpt(30, 17, 19, 50.0, 3, 0.50, 0.50, int(flags))


MEM_F_NOPAIRING, MEM_F_ALL, MEM_F_NO_MULTI, MEM_F_PRIMARY5, MEM_F_KEEP_SUPP_MAPQ = 0x4, 0x8, 0x10, 0x800, 0x1000
SEL_MAX_REGS = 512
SEL_DONE, SEL_TOO_MANY, SEL_SKIPPED = 0, 1, 2
SEL_NO_PAIRING, SEL_PAIRED = 0, 1
# bwagpu_pairsel_t
PAIRSEL_DTYPE = np.dtype([("status", "<i4"), ("branch", "<i4"), ("n_pri", "<i4", (2,)), ("z", "<i4", (2,)),
                          ("mapq", "<i4", (2,)), ("alt", "<i4", (2,)), ("extra_flag", "<i4"), ("o", "<i4"),
                          ("subo", "<i4"), ("n_sub", "<i4"), ("pad", "<i4", (2,))])
assert PAIRSEL_DTYPE.itemsize == 64 and C.sizeof(SelOpt) == 32


class SamOpt(C.Structure):
    """bwagpu_samopt_t: mem_opt_t's fields of mem_gen_alt's selection"""
    _fields_ = [("flags", C.c_int32), ("XA_drop_ratio", C.c_float), ("max_XA_hits", C.c_int32),
                ("max_XA_hits_alt", C.c_int32)]


def default_samopt(flags: int = 0) -> SamOpt:
    """mem_opt_init's defaults (bwa/bwamem.c:71-76)"""
    return SamOpt(int(flags), 0.80, 5, 200)


MEM_F_REF_HDR, MEM_F_SOFTCLIP, MEM_F_XB = 0x100, 0x200, 0x2000
SAM_DONE, SAM_SKIPPED, SAM_NEEDS_HOST, SAM_NO_ROOM = 0, 1, 2, 3
SAM_MAX_RG = 255


class SamText(C.Structure):
    """bwagpu_samtext_t: the arguments of bwagpu_sam_text_device (device pointers but rg_id)"""
    _fields_ = [(k, C.c_void_p) for k in (
        "dev_reg_off", "dev_regs", "dev_n", "dev_sel", "dev_out_mapq", "dev_xa_of", "dev_job_of", "dev_aln",
        "dev_cigar", "dev_md", "dev_seq_off", "dev_seq", "dev_qual", "dev_name_off", "dev_names", "dev_comment_off",
        "dev_comments", "dev_contig_off", "dev_contig_names")] + [
        ("rg_id", C.c_char_p), ("flags", C.c_int32), ("n_contigs", C.c_int32), ("job_cap", C.c_int32),
        ("max_ops", C.c_int32), ("max_md", C.c_int32), ("pad_", C.c_int32), ("text_cap", C.c_int64),
        ("dev_text", C.c_void_p), ("dev_text_off", C.c_void_p), ("dev_status", C.c_void_p),
        ("dev_text_n", C.c_void_p)]


assert C.sizeof(SamText) == 224


def default_chainopt() -> dict:
    """mem_opt_init's chaining defaults (bwa/bwamem.c:62-72)"""
    return dict(max_occ=500, max_chain_gap=10000, min_chain_weight=0, max_chain_extend=1 << 30, mask_level=0.5,
                drop_ratio=0.5)

# every entry point declared in include/bwagpu.h: name -> (restype, argtypes)
_VP = C.c_void_p
PROTOS = {
    "bwagpu_abi_version": (C.c_int, []),
    "bwagpu_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "bwagpu_create": (C.c_int, [C.c_int, C.POINTER(Opt), C.POINTER(Bns), _VP, C.POINTER(_VP)]),
    "bwagpu_create_resident": (C.c_int, [C.c_int, C.POINTER(Opt), C.POINTER(Bns), _VP, C.POINTER(_VP)]),
    "bwagpu_destroy": (C.c_int, [_VP]),
    "bwagpu_last_error": (C.c_char_p, [_VP]),
    "bwagpu_set_watchdog_ms": (C.c_int, [_VP, C.c_int]),
    "bwagpu_chain2aln_submit": (C.c_int, [_VP, C.c_int, C.POINTER(BatchC)]),
    "bwagpu_chain2aln_wait": (C.c_int, [_VP, C.c_int, _VP, _VP]),
    "bwagpu_chain2aln_stage": (C.c_int, [_VP, C.c_int, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                         C.POINTER(BatchC)]),
    "bwagpu_chain2aln_results": (C.c_int, [_VP, C.c_int, C.POINTER(_VP), C.POINTER(_VP)]),
    "bwagpu_chain2aln_results_dense": (C.c_int, [_VP, C.c_int, C.POINTER(_VP), C.POINTER(_VP), C.POINTER(_VP)]),
    "bwagpu_chain2aln": (C.c_int, [_VP, C.POINTER(BatchC), _VP, _VP]),
    "bwagpu_chain2aln_device": (C.c_int, [_VP, C.POINTER(BatchC), _VP, _VP, _VP, _VP]),
    "bwagpu_extend_batch": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int64, _VP, C.c_int64, _VP]),
    "bwagpu_align2_batch": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int64, _VP, C.c_int64, _VP]),
    "bwagpu_align2_device": (C.c_int, [_VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "bwagpu_reg2aln_batch": (C.c_int, [_VP, C.c_int32, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, _VP, _VP, _VP]),
    "bwagpu_reg2aln_device": (C.c_int, [_VP, C.c_int32, _VP, _VP, _VP, C.c_int64, C.c_int32, C.c_int32, _VP, _VP,
                                        _VP, _VP]),
    "bwagpu_reg2aln_jobs_device": (C.c_int, [_VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, C.c_int32, _VP, _VP, _VP, _VP]),
    "bwagpu_xa_select_device": (C.c_int, [_VP, C.POINTER(SamOpt), C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "bwagpu_sam_text_device": (C.c_int, [_VP, C.POINTER(SamText), C.c_int32, _VP]),
    "bwagpu_debug_sam_text_step": (C.c_int, [_VP, C.POINTER(SamText), C.c_int32, C.c_int32, _VP]),
    "bwagpu_debug_reg2aln_times": (C.c_int, [_VP, _VP]),
    "bwagpu_last_stats": (C.c_int, [_VP, C.c_int, C.POINTER(Stats)]),
    "bwagpu_debug_set_trace": (C.c_int, [_VP, _VP]),
    "bwagpu_prof_start": (C.c_int, [_VP, C.c_int]),
    "bwagpu_debug_fail_wait": (C.c_int, [_VP, C.c_int, C.c_int]),
    "bwagpu_debug_live_buffers": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "bwagpu_debug_spec_counters": (C.c_int, [_VP, _VP, _VP]),
    "bwagpu_debug_occupancy": (C.c_int, [_VP, _VP, _VP]),
    "bwagpu_debug_spec_ext": (C.c_int, [_VP, _VP, _VP, C.c_int32]),
    "bwagpu_prof_read": (C.c_int, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "bwagpu_prof_intervals": (C.c_int, [_VP, _VP, _VP, C.c_int32, C.POINTER(C.c_int32)]),
    "bwagpu_set_bwt": (C.c_int, [_VP, C.POINTER(BwtC)]),
    "bwagpu_debug_seed_budget": (C.c_int, [_VP, C.c_int32]),
    "bwagpu_debug_sup_shift": (C.c_int, [_VP, C.c_int32]),
    "bwagpu_set_device_read_len": (C.c_int, [_VP, C.c_int32]),
    "bwagpu_debug_ext_form": (C.c_int, [C.c_int]),
    "bwagpu_ctx_ext_form": (C.c_int, [_VP, C.c_int]),
    "bwagpu_ctx_ext_short": (C.c_int, [_VP, C.c_int]),
    "bwagpu_ctx_ext_short_fill": (C.c_int, [_VP, C.c_int]),
    "bwagpu_ctx_light_pack": (C.c_int, [_VP, C.c_int]),
    "bwagpu_debug_spec_short": (C.c_int, [_VP, _VP, _VP]),
    "bwagpu_ctx_row_bound": (C.c_int, [_VP, C.c_int]),
    "bwagpu_ctx_ungapped": (C.c_int, [_VP, C.c_int]),
    "bwagpu_debug_spec_ungapped": (C.c_int, [_VP, _VP, _VP]),
    "bwagpu_ctx_ungapped_right": (C.c_int, [_VP, C.c_int]),
    "bwagpu_debug_spec_ungapped_right": (C.c_int, [_VP, _VP, _VP]),
    "bwagpu_ctx_emu_finish": (C.c_int, [_VP, C.c_int]),
    "bwagpu_debug_spec_finish": (C.c_int, [_VP, _VP, _VP]),
    "bwagpu_ctx_fused_launches": (C.c_int, [_VP, C.c_int]),
    "bwagpu_debug_ext_kernel": (C.c_int, [_VP, C.c_int32]),
    "bwagpu_streams_concurrent": (C.c_int, [_VP, _VP]),
    "bwagpu_bwt_sa": (C.c_int, [_VP, C.c_int64, _VP, _VP]),
    "bwagpu_sw_stream": (C.c_int, [_VP, _VP, C.c_int64, _VP, C.c_int32, C.POINTER(C.c_int32)]),
    "bwagpu_collect_intv": (C.c_int, [_VP, C.POINTER(SeedOpt), C.c_int32, _VP, _VP, C.c_int32, _VP, C.c_int64,
                                       _VP]),
    "bwagpu_set_alt": (C.c_int, [_VP, _VP]),
    "bwagpu_seqs2chains": (C.c_int, [_VP, C.POINTER(SeedOpt), C.POINTER(ChainOpt), C.c_int32, _VP, _VP, C.c_int32,
                                      C.POINTER(ChainsC)]),
    "bwagpu_seqs2regions": (C.c_int, [_VP, C.POINTER(SeedOpt), C.POINTER(ChainOpt), C.c_int32, _VP, _VP, _VP,
                                       C.POINTER(_VP), C.POINTER(C.c_int64)]),
    "bwagpu_regs_post": (C.c_int, [_VP, C.POINTER(PostOpt), C.c_int32, C.c_int64, C.c_int32, _VP, _VP, _VP, _VP,
                                    _VP]),
    "bwagpu_regs_post_device": (C.c_int, [_VP, C.POINTER(PostOpt), C.c_int32, C.c_int64, C.POINTER(BatchC), _VP,
                                           _VP, _VP, _VP]),
    "bwagpu_set_regs_post": (C.c_int, [_VP, C.POINTER(PostOpt), C.c_int32, C.c_int64]),
    "bwagpu_pestat": (C.c_int, [_VP, C.POINTER(PairOpt), C.c_int32, _VP, _VP, _VP, _VP]),
    "bwagpu_pestat_device": (C.c_int, [_VP, C.POINTER(PairOpt), C.c_int32, _VP, _VP, _VP, _VP, _VP]),
    "bwagpu_mate_rescue": (C.c_int, [_VP, C.POINTER(PairOpt), _VP, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                      _VP, _VP]),
    "bwagpu_mate_rescue_device": (C.c_int, [_VP, C.POINTER(PairOpt), _VP, C.POINTER(BatchC), _VP, _VP, _VP, _VP, _VP,
                                             _VP, _VP, _VP, _VP]),
    "bwagpu_mark_primary": (C.c_int, [_VP, C.POINTER(SelOpt), C.c_int64, C.c_int32, _VP, _VP, _VP, _VP, _VP]),
    "bwagpu_mark_primary_device": (C.c_int, [_VP, C.POINTER(SelOpt), C.c_int64, C.c_int32, _VP, _VP, _VP, _VP, _VP,
                                              _VP]),
    "bwagpu_pair_select": (C.c_int, [_VP, C.POINTER(SelOpt), _VP, C.c_int64, C.c_int32, _VP, _VP, _VP, _VP, _VP, _VP,
                                      _VP]),
    "bwagpu_pair_select_device": (C.c_int, [_VP, C.POINTER(SelOpt), _VP, C.c_int64, C.c_int32, _VP, _VP, _VP, _VP,
                                             _VP, _VP, _VP, _VP]),
    "bwagpu_debug_rescue_drop": (C.c_int, [_VP, C.c_int32]),
    "bwagpu_debug_rescue_times": (C.c_int, [_VP, _VP]),
}

_lib = None


def lib_path() -> str:
    return os.environ.get("BWAGPU_LIB", os.path.join(LIB_DIR, "libbwagpu.so"))


def load() -> C.CDLL:
    """Load the HIP engine.  Fails loudly: there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    # one HIP runtime per process: when PyTorch is present its bundled
    # libamdhip64.so.7 must be the one our library binds to (same soname), so
    # import it first; a second runtime would hide the GPU from torch.
    if os.environ.get("BWAGPU_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    if not os.path.exists(p):
        raise RuntimeError(f"bwagpu: HIP engine library missing at {p}; run __graft_entry__.build()")
    lib = C.CDLL(p)
    for name, (res, args) in PROTOS.items():
        if (name.startswith("bwagpu_debug_") or name in ("bwagpu_ctx_light_pack", "bwagpu_ctx_ungapped", "bwagpu_ctx_ungapped_right", "bwagpu_ctx_emu_finish", "bwagpu_ctx_fused_launches")) and not hasattr(lib, name):
            continue  # an A/B build of an older tree (BWAGPU_LIB) may lack a newer diagnostic or A/B switch
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.bwagpu_abi_version() != ABI_VERSION:
        raise RuntimeError("bwagpu: ABI version mismatch")
    _lib = lib
    return lib


def opt_from_dict(d: dict) -> Opt:
    o = Opt()
    for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "pen_clip5", "pen_clip3", "w", "zdrop"):
        setattr(o, k, int(d[k]))
    mat = d.get("mat")
    if mat is None:
        mat = fill_scmat(int(d["a"]), int(d["b"]))
    for i in range(25):
        o.mat[i] = int(mat[i])
    return o


def fill_scmat(a: int, b: int) -> np.ndarray:
    """bwa_fill_scmat (bwa/bwa.c:109-118): a on the diagonal, -b off it, -1 for N."""
    m = np.full((5, 5), -1, np.int8)
    for i in range(4):
        for j in range(4):
            m[i, j] = a if i == j else -b
    return m.reshape(-1)


def default_opt() -> dict:
    """mem_opt_init defaults (bwa/bwamem.c:48-84)."""
    return dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, pen_clip5=5, pen_clip3=5, w=100,
                zdrop=100, mat=fill_scmat(1, 4))
