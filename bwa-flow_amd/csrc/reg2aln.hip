// reg2aln.hip — MI355X (gfx950) CIGAR generation of bwa-flow's SAM stage:
// mem_reg2aln (bwa/bwamem.c:1104-1174) per output region, i.e. infer_bw
// (801-808), the band-doubling loop (1123-1134) over bwa_gen_cigar2
// (bwa/bwa.c:121-207) and its banded global DP with backtrack ksw_global2
// (bwa/ksw.c:504-606), NM and the MD string, the deletion squeeze, soft clips
// and the contig position (bwamem.c:1137-1166, bntseq.h:87-90,
// bntseq.c:349-363).  Called from src/bwa_wrapper.cpp:611/728/736/774.
//
// One wave per region (job):
//  * the query slice and the reference window (2-bit pac gather, reverse
//    strand = complement of the mirrored forward strand; both sequences
//    reversed for reverse-strand regions, bwa.c:136-141) go to LDS once and
//    serve every band try;
//  * DP rows over the target; query columns STRIDED over the lanes (lane r
//    holds eh[] slots j = 64c + r, c < CD), exactly the reference's eh[]
//    update per row: M from the slot's own H(i-1, j-1), E from the slot, F as
//    an exclusive max-plus scan (F_j = max(NEG - (j-lo)e, max_{lo<=k<j}
//    (M_k - oe_ins + k e) - (j-1) e)), the slot's new H(i, j-1) by a one-lane
//    shift; every in-band cell writes its direction byte (h source | E flag
//    << 2 | F flag << 4, ksw.c:552-566) to a row-major ncol-stride matrix in
//    LDS (or, for jobs whose matrix exceeds the LDS bins, in a per-wave HBM
//    slice);
//  * the backtrack (ksw.c:578-590) walks that matrix with the reference's
//    state-dependent bit shift; runs are merged as push_cigar does;
//  * MD/NM: matched runs compared 64 bases per step, mismatches from a ballot.
#include <hip/hip_runtime.h>

#include "block_scan.h"
#include "engine.h"
#include "global_dp.h"
#include "reg2aln.h"
#include "wave_ops.h"

namespace bwagpu {

namespace {

// infer_bw, bwamem.c:801-808
__device__ int infer_bw_dev(int l1, int l2, int score, int a, int q, int r) {
  if (l1 == l2 && l1 * a - score < (q + r - a) << 1) return 0;
  int w = (int)((double)((l1 < l2 ? l1 : l2) * a - score - q) / r + 2.);
  const int d = l1 > l2 ? l1 - l2 : l2 - l1;
  return w < d ? d : w;
}

__device__ __forceinline__ void put_md_int(char* md, int& ml, int cap, int v, bool& ovf) {
  char b[12];
  int n = 0;
  do {
    b[n++] = (char)('0' + v % 10);
    v /= 10;
  } while (v);
  if (ml + n >= cap) {
    ovf = true;
    return;
  }
  while (n) md[ml++] = b[--n];
}
__device__ __forceinline__ void put_md_chr(char* md, int& ml, int cap, char ch, bool& ovf) {
  if (ml + 1 >= cap) {
    ovf = true;
    return;
  }
  md[ml++] = ch;
}

}  // namespace

template <int CD>
__global__ void __launch_bounds__(256) reg2aln_kernel(DevOpt o, DevRef ref, R2AArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int lane = (int)(threadIdx.x & 63);
  const int wib = uni((int)(threadIdx.x >> 6)), wpb = (int)(blockDim.x >> 6);
  const int wave = (int)blockIdx.x * wpb + wib, nwaves = (int)gridDim.x * wpb;
  uint8_t* const wl = lds + (size_t)wib * a.lds_per_wave;
  uint8_t* const q = wl;                                               // qcap bytes
  uint8_t* const r = wl + a.qcap;                                      // rcap bytes
  uint32_t* const ops = reinterpret_cast<uint32_t*>(wl + a.qcap + a.rcap);  // ocap words
  uint8_t* const z = a.zglob ? a.zglob + (int64_t)wave * a.zstride : wl + a.qcap + a.rcap + 4 * a.ocap;
  const int64_t l_pac = ref.l_pac, two = l_pac << 1;
  const int wmax = o.w << 2;
  int64_t t_cells = 0, t_rows = 0, t_calls = 0;
  const int n_jobs = a.dev_n ? min(a.n, uni(*a.dev_n)) : a.n;
  for (int li = wave; li < n_jobs; li += nwaves) {
    const int k = uni(a.list[li]);
    const bwagpu_reg2aln_task_t* tp = a.tasks + k;
    const int64_t rb = uni64(tp->rb), re = uni64(tp->re), qoff = uni64(tp->qoff);
    const int l_seq = uni(tp->l_seq), qb = uni(tp->qb), qe = uni(tp->qe), truesc = uni(tp->truesc),
              wreg = uni(tp->w);
    bwagpu_aln_t res{};
    if (rb < 0 || re < 0) {  // bwamem.c:1112-1115
      res.rid = -1;
      res.pos = -1;
      res.status = BWAGPU_ALN_UNMAPPED;
      if (lane == 0) a.out[k] = res;
      continue;
    }
    const int lq = qe - qb;
    const int64_t rl64 = re - rb;
    // bwa_gen_cigar2's rejections (bwa.c:133-135): none depends on the band
    const int64_t beg = rb < 0 ? 0 : rb, end = re > two ? two : re;
    if (lq <= 0 || rb >= re || (rb < l_pac && re > l_pac) || !(beg >= l_pac || end <= l_pac) || end - beg != rl64) {
      int w2 = max(infer_bw_dev(lq, (int)rl64, truesc, o.a, o.o_del, o.e_del),
                   infer_bw_dev(lq, (int)rl64, truesc, o.a, o.o_ins, o.e_ins));
      if (w2 > o.w) w2 = min(w2, wreg);
      res.w = min(w2, wmax);
      res.NM = -1;
      res.status = BWAGPU_ALN_NO_CIGAR;
      t_calls += 1;
      if (lane == 0) a.out[k] = res;
      continue;
    }
    const int rl = (int)rl64;
    const bool rev = rb >= l_pac;
    // query slice and reference window into LDS (reversed for the reverse strand)
    for (int x = lane; x < lq; x += 64) q[x] = a.qpool[qoff + qb + (rev ? lq - 1 - x : x)];
    for (int x = lane; x < rl; x += 64) {
      const int64_t p = rev ? re - 1 - x : rb + x;
      const int64_t f = p >= l_pac ? two - 1 - p : p;
      const int b = (ref.pac[f >> 2] >> ((~f & 3) << 1)) & 3;
      r[x] = (uint8_t)(p >= l_pac ? 3 - b : b);
    }
    wave_sync_lds();
    // the band loop (bwamem.c:1122-1134)
    int w2 = max(infer_bw_dev(lq, rl, truesc, o.a, o.o_del, o.e_del),
                 infer_bw_dev(lq, rl, truesc, o.a, o.o_ins, o.e_ins));
    if (w2 > o.w) w2 = min(w2, wreg);
    int last = -(1 << 30), score = 0, wcall = 0, tries = 0, wdp = 0, ncol = 0;
    bool ungapped = false;
    for (;;) {
      w2 = min(w2, wmax);
      wcall = w2;
      t_calls += 1;
      if (lq == rl && w2 == 0) {  // bwa.c:142-150
        int s = 0;
        for (int x = lane; x < lq; x += 64) s += o.mat[r[x] * 5 + q[x]];
        score = wave_sum(s);
        ungapped = true;
      } else {  // bwa.c:152-165
        const int half = (lq + 1) >> 1;
        const int mi = (int)((double)(half * o.mat[0] - o.o_ins) / o.e_ins + 1.);
        const int md = (int)((double)(half * o.mat[0] - o.o_del) / o.e_del + 1.);
        int mg = max(max(mi, md), 1);
        const int dl = lq > rl ? lq - rl : rl - lq;
        int w = min((mg + dl + 1) >> 1, w2);
        w = max(w, dl + 3);
        wdp = w;
        ncol = lq < 2 * w + 1 ? lq : 2 * w + 1;
        ungapped = false;
        if (2 * w + 1 <= 64)
          score = uni(band_dp<1>(o, lq, q, rl, r, w, ncol, z, t_cells));
        else if (2 * w + 1 <= 128 && CD >= 2)
          score = uni(band_dp<(CD >= 2 ? 2 : 1)>(o, lq, q, rl, r, w, ncol, z, t_cells));
        else
          score = uni(global_dp<CD>(o, lq, q, rl, r, w, ncol, z, t_cells));
        t_rows += rl;
      }
      if (score == last || w2 == wmax) break;
      last = score;
      w2 <<= 1;
      if (!(++tries < 3 && score < truesc - o.a)) break;
    }
    res.score = score;
    res.w = wcall;
    // ---- CIGAR of the last try: backtrack (ksw.c:578-590), reversed runs in ops[]
    int nops = 0;
    if (ungapped) {
      if (lane == 0) ops[0] = (uint32_t)lq << 4;
      nops = 1;
    } else {
      wave_sync_lds();  // direction bytes of every lane visible
      // Runs of one state are taken 64 cells at a time: in state s the walk
      // moves diagonally (s = 0, M), up (1, D) or left (2, I) and stays in s
      // while the cell's bits for s (>> 2s) read s again; lane l looks at the
      // l-th cell of the run, a ballot finds where it ends.  Cells outside the
      // row's band end a run (the serial step then reads what the reference
      // reads).
      int i = rl - 1, kk = min(i + wdp + 1, lq) - 1, st = 0, cop = -1, clen = 0;
      auto emit = [&](int op, int len) {
        if (op == cop) {
          clen += len;
        } else {
          if (clen && lane == 0) ops[nops] = (uint32_t)clen << 4 | (uint32_t)cop;
          nops += clen ? 1 : 0;
          cop = op;
          clen = len;
        }
      };
      while (i >= 0 && kk >= 0) {
        const int di = st != 2, dk = st != 1;
        const int il = i - lane * di, kl = kk - lane * dk;
        const int lol = il > wdp ? il - wdp : 0, hil = min(il + wdp + 1, lq);
        const bool valid = il >= 0 && kl >= lol && kl < hil;
        const int d = valid ? (int)z[(size_t)il * ncol + (kl - lol)] : 0;
        const bool stop = !valid || ((d >> (st << 1)) & 3) != st;
        const uint64_t sb = __builtin_amdgcn_ballot_w64(stop);
        const int f = sb ? __builtin_ctzll(sb) : 64;
        if (f) {
          emit(st == 0 ? 0 : (st == 1 ? 2 : 1), f);
          i -= f * di;
          kk -= f * dk;
        }
        if (f < 64 && i >= 0 && kk >= 0) {  // one serial step at the run's end (reference addressing)
          const int lo_i = i > wdp ? i - wdp : 0;
          // a walk that leaves the band reads outside the row in the reference
          // (undefined there); here the index stays inside the matrix
          int64_t zi = (int64_t)i * ncol + (kk - lo_i);
          zi = zi < 0 ? 0 : (zi >= (int64_t)ncol * rl ? (int64_t)ncol * rl - 1 : zi);
          const int dd = uni((int)z[zi]);
          st = (dd >> (st << 1)) & 3;
          emit(st == 0 ? 0 : (st == 1 ? 2 : 1), 1);
          i -= st != 2;
          kk -= st != 1;
        }
      }
      auto push = emit;
      // the ends (ksw.c:591-592), then the last run
      if (i >= 0) push(2, i + 1);
      if (kk >= 0) push(1, kk + 1);
      if (clen && lane == 0) ops[nops] = (uint32_t)clen << 4 | (uint32_t)cop;
      nops += clen ? 1 : 0;
      // forward order
      for (int x = lane; x < nops >> 1; x += 64) {
        const uint32_t t0 = ops[x];
        ops[x] = ops[nops - 1 - x];
        ops[nops - 1 - x] = t0;
      }
    }
    wave_sync_lds();
    // ---- NM and MD (bwa.c:167-199), MD written straight to the job's slot
    char* const mdo = a.md + (int64_t)k * a.max_md;
    const bool fwd = rb < l_pac;
    int x = 0, y = 0, u = 0, nmm = 0, ngap = 0, ml = 0;
    bool ovf = false;
    for (int kop = 0; kop < nops; ++kop) {
      const uint32_t cv = uni((int)ops[kop]);
      const int op = (int)(cv & 0xf), len = (int)(cv >> 4);
      if (op == 0) {
        for (int s0 = 0; s0 < len; s0 += 64) {
          const int n = min(64, len - s0);
          const bool mm = lane < n && q[x + s0 + lane] != r[y + s0 + lane];
          uint64_t bits = __builtin_amdgcn_ballot_w64(mm);
          int cur = 0;
          while (bits) {
            const int b = __builtin_ctzll(bits);
            bits &= bits - 1;
            u += b - cur;
            const int rbse = uni((int)r[y + s0 + b]);
            if (lane == 0) {
              put_md_int(mdo, ml, a.max_md, u, ovf);
              put_md_chr(mdo, ml, a.max_md, "ACGTN"[fwd ? rbse : (rbse < 4 ? 3 - rbse : 4)], ovf);
            }
            ++nmm;
            u = 0;
            cur = b + 1;
          }
          u += n - cur;
        }
        x += len;
        y += len;
      } else if (op == 2) {
        if (kop > 0 && kop < nops - 1) {
          if (lane == 0) {
            put_md_int(mdo, ml, a.max_md, u, ovf);
            put_md_chr(mdo, ml, a.max_md, '^', ovf);
            for (int b = 0; b < len; ++b) {
              const int rbse = r[y + b];
              put_md_chr(mdo, ml, a.max_md, "ACGTN"[fwd ? rbse : (rbse < 4 ? 3 - rbse : 4)], ovf);
            }
          }
          u = 0;
          ngap += len;
        }
        y += len;
      } else if (op == 1) {
        x += len;
        ngap += len;
      }
    }
    if (lane == 0) {
      put_md_int(mdo, ml, a.max_md, u, ovf);
      if (!ovf) mdo[ml] = 0;
    }
    ovf = uni(ovf ? 1 : 0) != 0;
    ml = uni(ml);
    res.NM = nmm + ngap;
    // ---- squeeze / clip / position (bwamem.c:1137-1166)
    int64_t pos = rb < l_pac ? rb : re - 1;
    const int is_rev = pos >= l_pac;
    if (is_rev) pos = two - 1 - pos;
    int s0 = 0, n = nops;
    if (n > 0) {
      const uint32_t f0 = uni((int)ops[0]), fl = uni((int)ops[n - 1]);
      if ((f0 & 0xf) == 2) {
        pos += f0 >> 4;
        s0 = 1;
        --n;
      } else if ((fl & 0xf) == 2) {
        --n;
      }
    }
    int clip5 = 0, clip3 = 0;
    if (qb != 0 || qe != l_seq) {
      clip5 = is_rev ? l_seq - qe : qb;
      clip3 = is_rev ? qb : l_seq - qe;
    }
    const int total = n + (clip5 != 0) + (clip3 != 0);
    if (ovf || total > a.max_ops) {
      res.status = BWAGPU_ALN_OVERFLOW;
      if (lane == 0) a.out[k] = res;
      continue;
    }
    uint32_t* const co = a.cigar + (int64_t)k * a.max_ops;
    const int c0 = clip5 != 0;
    for (int e = lane; e < n; e += 64) co[c0 + e] = ops[s0 + e];
    if (lane == 0) {
      if (clip5) co[0] = (uint32_t)clip5 << 4 | 3;
      if (clip3) co[c0 + n] = (uint32_t)clip3 << 4 | 3;
    }
    // bns_pos2rid (bntseq.c:349-363)
    int left = 0, mid = 0, right = ref.n_seqs;
    if (pos >= l_pac) {
      mid = -1;
    } else {
      while (left < right) {
        mid = (left + right) >> 1;
        if (pos >= ref.ann_offset[mid]) {
          if (mid == ref.n_seqs - 1) break;
          if (pos < ref.ann_offset[mid + 1]) break;
          left = mid + 1;
        } else {
          right = mid;
        }
      }
    }
    res.rid = mid;
    res.pos = mid >= 0 ? pos - ref.ann_offset[mid] : pos;
    res.is_rev = is_rev;
    res.n_cigar = total;
    res.md_len = ml;
    res.status = BWAGPU_ALN_OK;
    if (lane == 0) a.out[k] = res;
  }
  if (a.stats && lane == 0) {
    if (t_cells) atomicAdd((unsigned long long*)&a.stats[ST_CELLS], (unsigned long long)t_cells);
    if (t_rows) atomicAdd((unsigned long long*)&a.stats[ST_ROWS], (unsigned long long)t_rows);
    if (t_calls) atomicAdd((unsigned long long*)&a.stats[ST_CALLS], (unsigned long long)t_calls);
  }
}

// ---------------------------------------------------------------- bwagpu_reg2aln_device
// A lane per job: r2_classify (pure.h) decides; a refused job gets its record
// here and no key.  Counts and maxima are gathered per workgroup in LDS and
// leave it as one atomic per word that is not zero.
__global__ void __launch_bounds__(256) reg2aln_classify_kernel(DevOpt o, int64_t l_pac, int64_t qpool_len, int n_cap,
                                                               const int32_t* __restrict__ dev_n_tasks,
                                                               const bwagpu_reg2aln_task_t* __restrict__ tasks,
                                                               int32_t* __restrict__ keys,
                                                               bwagpu_aln_t* __restrict__ out,
                                                               int32_t* __restrict__ table) {
  __shared__ int32_t tab[kR2TabWords];
  for (int x = (int)threadIdx.x; x < kR2TabWords; x += (int)blockDim.x) tab[x] = 0;
  __syncthreads();
  int n = n_cap;
  if (dev_n_tasks) n = max(0, min(n_cap, *dev_n_tasks));
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // n_cap may be near INT_MAX
  if (k < n_cap) {
    int key = -1;
    if (k < n) {
      const R2Class c = r2_classify(o, l_pac, qpool_len, tasks[k]);
      if (c.verdict == R2_ACCEPTED) {
        const int bin = c.bucket * 3 + c.cls;
        key = bin * kR2CostClasses + r2_cost_class(c.cls, c.zb + c.lq + c.rl);
        atomicAdd(&tab[4 * bin], 1);
        atomicMax(&tab[4 * bin + 1], c.lq);
        atomicMax(&tab[4 * bin + 2], c.rl);
        atomicMax(&tab[4 * bin + 3], (int32_t)c.zb);  // <= 1023 * 8192
        atomicAdd(&tab[kR2TabClass + key], 1);
      } else {
        bwagpu_aln_t res{};
        res.rid = -1;
        res.pos = -1;
        res.status = BWAGPU_ALN_REFUSED;
        out[k] = res;
        atomicAdd(&tab[kR2TabRefused], 1);
      }
    }
    keys[k] = key;
  }
  __syncthreads();
  for (int x = (int)threadIdx.x; x < kR2TabJobs; x += (int)blockDim.x) {
    const int32_t v = tab[x];
    if (!v) continue;
    if (x < kR2TabClass && (x & 3)) atomicMax(&table[x], v);
    else atomicAdd(&table[x], v);
  }
  if (threadIdx.x == 0) {
    if (tab[kR2TabRefused]) atomicAdd(&table[kR2TabRefused], tab[kR2TabRefused]);
    if (blockIdx.x == 0) table[kR2TabJobs] = n;
  }
}

// Job ids into the one list, every (bin, cost class) from its offset on: one
// atomic per distinct key per wave.  The order inside a key is free.
__global__ void __launch_bounds__(256) reg2aln_scatter_kernel(int n_cap, const int32_t* __restrict__ keys, R2Offsets off,
                                                              int32_t* __restrict__ cursors,
                                                              int32_t* __restrict__ list) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const int key = k < n_cap ? keys[k] : -1;
  const bool live = key >= 0 && key < kR2Bins * kR2CostClasses;
  unsigned long long todo = __builtin_amdgcn_ballot_w64(live);
  while (todo) {
    const int leader = __builtin_ctzll(todo);
    const int b = __builtin_amdgcn_readlane(key, leader);
    const unsigned long long m = __builtin_amdgcn_ballot_w64(live && key == b);
    int pos0 = 0;
    if (lane == leader) pos0 = atomicAdd(&cursors[b], __builtin_popcountll(m));
    pos0 = __builtin_amdgcn_readlane(pos0, leader);
    if (live && key == b) list[off.at[b] + pos0 + __builtin_popcountll(m & ((1ull << lane) - 1))] = (int32_t)k;
    todo &= ~m;
  }
}

hipError_t launch_reg2aln_classify(const DevOpt& o, int64_t l_pac, int64_t qpool_len, int n_cap,
                                   const int32_t* dev_n_tasks, const bwagpu_reg2aln_task_t* tasks, int32_t* keys,
                                   bwagpu_aln_t* out, int32_t* table, hipStream_t st) {
  hipLaunchKernelGGL(reg2aln_classify_kernel, dim3((unsigned)(((int64_t)n_cap + 255) / 256)), dim3(256), 0, st, o, l_pac, qpool_len, n_cap,
                     dev_n_tasks, tasks, keys, out, table);
  return hipGetLastError();
}

hipError_t launch_reg2aln_scatter(int n_cap, const int32_t* keys, const R2Offsets& off, int32_t* cursors,
                                  int32_t* list, hipStream_t st) {
  hipLaunchKernelGGL(reg2aln_scatter_kernel, dim3((unsigned)(((int64_t)n_cap + 255) / 256)), dim3(256), 0, st, n_cap, keys, off, cursors,
                     list);
  return hipGetLastError();
}

// ---------------------------------------------------------------- bwagpu_reg2aln_jobs_device
namespace {

__device__ __forceinline__ int r2j_count(int r, int n_reads, const int64_t* reg_off, const int32_t* n,
                                         const int32_t* select) {
  if (r >= n_reads) return 0;
  const int64_t base = reg_off[r];
  int c = 0;
  for (int k = 0; k < n[r]; ++k) c += select[base + k] >= 0;
  return c;
}

}  // namespace

__global__ void __launch_bounds__(256) reg2aln_jobs_count_kernel(int n_reads, const int64_t* __restrict__ reg_off,
                                                                 const int32_t* __restrict__ n,
                                                                 const int32_t* __restrict__ select,
                                                                 int32_t* __restrict__ block_sums) {
  const int r = (int)min((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)n_reads);  // n_reads: no read
  int total = 0;
  (void)block_excl_scan(r2j_count(r, n_reads, reg_off, n, select), &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// one workgroup: block_sums -> their exclusive prefix, in place; the two counts
__global__ void __launch_bounds__(256) reg2aln_jobs_scan_kernel(int n_blocks, int job_cap,
                                                                int32_t* __restrict__ block_sums,
                                                                int32_t* __restrict__ n_jobs) {
  int carry = 0;
  for (int x0 = 0; x0 < n_blocks; x0 += 256) {
    const int x = x0 + (int)threadIdx.x;
    const int v = x < n_blocks ? block_sums[x] : 0;
    int total = 0;
    const int ex = block_excl_scan(v, &total);
    if (x < n_blocks) block_sums[x] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    n_jobs[0] = min(carry, job_cap);
    n_jobs[1] = carry;
  }
}

__global__ void __launch_bounds__(256) reg2aln_jobs_write_kernel(int n_reads, const int64_t* __restrict__ reg_off,
                                                                 const bwagpu_alnreg_t* __restrict__ regs,
                                                                 const int32_t* __restrict__ n,
                                                                 const int32_t* __restrict__ select,
                                                                 const int64_t* __restrict__ seq_off, int job_cap,
                                                                 bwagpu_reg2aln_task_t* __restrict__ tasks,
                                                                 int32_t* __restrict__ job_of,
                                                                 const int32_t* __restrict__ block_sums) {
  const int r = (int)min((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)n_reads);  // n_reads: no read
  int total = 0;
  int j = block_sums[blockIdx.x] + block_excl_scan(r2j_count(r, n_reads, reg_off, n, select), &total);
  if (r >= n_reads) return;
  const int64_t base = reg_off[r], qoff = seq_off[r];
  const int l_seq = (int)(seq_off[r + 1] - qoff);
  for (int k = 0; k < n[r]; ++k) {
    if (select[base + k] < 0) {
      job_of[base + k] = -1;
      continue;
    }
    if (j < job_cap) {
      const bwagpu_alnreg_t& g = regs[base + k];
      bwagpu_reg2aln_task_t t{};
      t.rb = g.rb, t.re = g.re, t.qoff = qoff, t.l_seq = l_seq, t.qb = g.qb, t.qe = g.qe, t.truesc = g.truesc,
      t.w = g.w;
      tasks[j] = t;
    }
    job_of[base + k] = j < job_cap ? j : -1;
    ++j;
  }
}

hipError_t launch_reg2aln_jobs(int n_reads, const int64_t* reg_off, const bwagpu_alnreg_t* regs, const int32_t* n,
                               const int32_t* select, const int64_t* seq_off, int job_cap,
                               bwagpu_reg2aln_task_t* tasks, int32_t* job_of, int32_t* n_jobs, int32_t* block_sums,
                               hipStream_t st) {
  const int nb = (int)(((int64_t)n_reads + 255) / 256);
  hipLaunchKernelGGL(reg2aln_jobs_count_kernel, dim3(nb), dim3(256), 0, st, n_reads, reg_off, n, select, block_sums);
  hipLaunchKernelGGL(reg2aln_jobs_scan_kernel, dim3(1), dim3(256), 0, st, nb, job_cap, block_sums, n_jobs);
  hipLaunchKernelGGL(reg2aln_jobs_write_kernel, dim3(nb), dim3(256), 0, st, n_reads, reg_off, regs, n, select, seq_off,
                     job_cap, tasks, job_of, block_sums);
  return hipGetLastError();
}

int r2_resident_waves(int cd, size_t lds_per_block, int wpb) {
  int dev = 0, ncu = 0, per = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 4096;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 4096;
  hipError_t e = hipErrorInvalidValue;
  switch (cd) {
#define R2_OCC(C) \
  case C: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, reg2aln_kernel<C>, 64 * wpb, lds_per_block); break;
    R2_OCC(1) R2_OCC(2) R2_OCC(3) R2_OCC(4) R2_OCC(8) R2_OCC(16)
#undef R2_OCC
  }
  if (e != hipSuccess || per < 1) per = 1;
  return per * ncu * wpb;
}

hipError_t launch_reg2aln(int cd, const DevOpt& o, const DevRef& ref, const R2AArgs& a, int n_blocks, int wpb,
                          hipStream_t st) {
  const size_t lds = (size_t)wpb * a.lds_per_wave;
  switch (cd) {
#define R2_LAUNCH(C)                                                                                   \
  case C:                                                                                              \
    hipLaunchKernelGGL((reg2aln_kernel<C>), dim3(n_blocks), dim3(64 * wpb), lds, st, o, ref, a);            \
    return hipGetLastError();
    R2_LAUNCH(1) R2_LAUNCH(2) R2_LAUNCH(3) R2_LAUNCH(4) R2_LAUNCH(8) R2_LAUNCH(16)
#undef R2_LAUNCH
  }
  return hipErrorInvalidValue;
}

}  // namespace bwagpu
