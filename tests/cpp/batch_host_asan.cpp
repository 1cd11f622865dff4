// batch_host_asan.cpp — the host-side passes over a batch: chain2aln's checks
// and staging copy (bwa-flow_amd/csrc/batch_host.h), seeding's checks, staging
// copy and gate table (seed_host.h) and the pass pool (host_pool.h) under the
// host sanitizers.  Stand-alone: no GPU, no HIP, not loaded into any other
// process.
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
//       -I include -I bwa-flow_amd/csrc tests/cpp/batch_host_asan.cpp -o batch_host_asan && ./batch_host_asan
//   ... and once more with -fsanitize=thread
//
// Every array handed to a pass is a heap allocation of exactly the size the
// batch header declares, and the staging buffers are exactly as large as the
// passes may fill, so a read or write past them is an AddressSanitizer report.
#include <math.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "batch_host.h"
#include "seed_host.h"

using namespace bwagpu;

static int g_fail = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                   \
    }                                                             \
  } while (0)

template <class T>
static T* exact(size_t n) {  // n elements and not a byte more (nothing for none)
  return n ? (T*)std::malloc(n * sizeof(T)) : nullptr;
}

static const int64_t kLPac = (int64_t)1 << 30;

// ------------------------------------------------------------- chain2aln batch
// nr reads of len(r) bases, one chain per read, one seed per chain
struct Batch {
  bwagpu_batch_t b{};
  int64_t* so;
  uint8_t* seq;
  int32_t *rco, *cso, *rid;
  float* frac;
  bwagpu_seed_t* sd;
  InLayout L;
  char* h;  // the staging buffer, exactly L.total bytes

  Batch(int nr, const std::function<int(int)>& len) {
    int64_t sb = 0;
    for (int r = 0; r < nr; ++r) sb += len(r);
    so = exact<int64_t>((size_t)nr + 1), rco = exact<int32_t>((size_t)nr + 1), cso = exact<int32_t>((size_t)nr + 1);
    rid = exact<int32_t>((size_t)nr), frac = exact<float>((size_t)nr), sd = exact<bwagpu_seed_t>((size_t)nr);
    seq = exact<uint8_t>((size_t)sb);
    so[0] = 0;
    for (int r = 0; r < nr; ++r) {
      so[r + 1] = so[r] + len(r);
      rid[r] = r % 3, frac[r] = 0.25f * (float)(r % 5);
      sd[r] = bwagpu_seed_t{3 * (int64_t)r, 1, 10, 10, 0};
    }
    for (int r = 0; r <= nr; ++r) rco[r] = cso[r] = r;
    for (int64_t i = 0; i < sb; ++i) seq[i] = (uint8_t)((i * 7 + i / 5) % 5);
    b.n_reads = b.n_chains = b.n_seeds = nr;
    b.seq_bytes = sb;
    b.seq_off = so, b.seq = seq, b.read_chain_off = rco, b.chain_seed_off = cso, b.chain_rid = rid;
    b.chain_frac_rep = frac, b.seeds = sd;
    L.make(b);
    h = exact<char>(L.total);
  }
  ~Batch() {
    for (void* p : {(void*)so, (void*)seq, (void*)rco, (void*)cso, (void*)rid, (void*)frac, (void*)sd, (void*)h})
      std::free(p);
  }
  Batch(const Batch&) = delete;
};

struct Verdict {
  int rc = 0, lq = 0;
  std::string why;
  bool operator==(const Verdict& o) const { return rc == o.rc && lq == o.lq && why == o.why; }
  bool is(int code, const char* text) const { return rc == code && why == text; }
};

static Verdict staged(Batch& x) {  // what bwagpu_chain2aln_submit runs on a caller's arrays
  Verdict v;
  if ((v.rc = check_batch_header(&x.b, &v.why))) return v;
  v.rc = stage_and_check(&x.b, kLPac, x.h, x.L, &v.lq, &v.why);
  return v;
}
static Verdict checked(Batch& x) {  // ... and on a batch packed into the staging buffer by the caller
  Verdict v;
  if ((v.rc = check_batch_header(&x.b, &v.why))) return v;
  v.rc = check_batch_seeds(&x.b, kLPac, &v.lq, &v.why);
  return v;
}
static Verdict sequential(Batch& x) {  // one check_reads over the whole batch
  Verdict v;
  int code = 0, bad_read = 0;
  int64_t lm = 0;
  code = check_reads(&x.b, kLPac, 0, x.b.n_reads, &lm, &bad_read);
  if (!(v.rc = check_report(&x.b, &code, &bad_read, 1, &v.why))) v.lq = (int)lm;
  return v;
}

// one value of one array changed for the length of a scope
template <class T>
struct Poke {
  T* at;
  T old;
  Poke(const T* p, T v) : at(const_cast<T*>(p)), old(*p) { *at = v; }
  ~Poke() { *at = old; }
  Poke(const Poke&) = delete;
};

static int len_small(int r) { return 20 + r % 7; }

static const char* kSeqOff = "seq_off not monotone";
static const char* kRco = "read_chain_off not monotone";
static const char* kCso = "chain_seed_off not monotone";
static const char* kSeed = "seed outside its read or the reference";

static void expect_all(Batch& x, int code, const char* text) {
  const Verdict s = staged(x), c = checked(x), q = sequential(x);
  EXPECT(s.is(code, text));
  EXPECT(c.is(code, text));
  EXPECT(q.is(code, text));
}

// every check_reads code with its defect on read r (0 < r < n_reads - 1) of x
static void defects_on_read(Batch& x, int r) {
  const bwagpu_batch_t& b = x.b;
  const int32_t nc = b.n_chains, ns = b.n_seeds;
  const int64_t l = b.seq_off[r + 1] - b.seq_off[r];
  {  // code 1: read r has length -1
    Poke<int64_t> p(b.seq_off + r, b.seq_off[r + 1] + 1);
    expect_all(x, BWAGPU_E_INVAL, kSeqOff);
  }
  // code 3: read_chain_off decreasing, negative, past n_chains
  for (int32_t v : {b.read_chain_off[r + 1] + 1, -5, nc + 1}) {
    Poke<int32_t> p(b.read_chain_off + r, v);
    expect_all(x, BWAGPU_E_INVAL, kRco);
  }
  // code 4: the same for chain_seed_off (chain r is read r's)
  for (int32_t v : {b.chain_seed_off[r + 1] + 1, -5, ns + 1}) {
    Poke<int32_t> p(b.chain_seed_off + r, v);
    expect_all(x, BWAGPU_E_INVAL, kCso);
  }
  // code 5: seed r is read r's
  const bwagpu_seed_t good = b.seeds[r];
  bwagpu_seed_t bad[5] = {good, good, good, good, good};
  bad[0].qbeg = -1;
  bad[1].len = 0;
  bad[2].qbeg = (int32_t)l - good.len + 1;  // qbeg + len = l + 1
  bad[3].rbeg = -1;
  bad[4].rbeg = 2 * kLPac - good.len + 1;  // rbeg + len = 2 * l_pac + 1
  for (const bwagpu_seed_t& s : bad) {
    Poke<bwagpu_seed_t> p(b.seeds + r, s);
    expect_all(x, BWAGPU_E_INVAL, kSeed);
  }
  {  // the largest seed that fits is accepted
    bwagpu_seed_t s = good;
    s.qbeg = (int32_t)l - good.len, s.rbeg = 2 * kLPac - good.len;
    Poke<bwagpu_seed_t> p(b.seeds + r, s);
    EXPECT(staged(x).rc == BWAGPU_OK && checked(x).rc == BWAGPU_OK);
  }
}

// code 2: a batch of nr reads whose read r has BWAGPU_MAX_READ_LEN + 1 bases, then exactly BWAGPU_MAX_READ_LEN
static void long_read(int nr, int r) {
  {
    Batch x(nr, [r](int k) { return k == r ? BWAGPU_MAX_READ_LEN + 1 : len_small(k); });
    char want[64];
    std::snprintf(want, sizeof want, "read %d has length %d > %d", r, BWAGPU_MAX_READ_LEN + 1, BWAGPU_MAX_READ_LEN);
    expect_all(x, BWAGPU_E_UNSUPPORTED, want);
  }
  Batch x(nr, [r](int k) { return k == r ? BWAGPU_MAX_READ_LEN : len_small(k); });
  const Verdict s = staged(x);
  EXPECT(s.rc == BWAGPU_OK && s.lq == BWAGPU_MAX_READ_LEN);
  EXPECT(s == checked(x) && s == sequential(x));
}

static void header_cases() {
  Batch x(3, len_small);
  bwagpu_batch_t& b = x.b;
  std::string why;
  EXPECT(check_batch_header(nullptr, &why) == BWAGPU_E_INVAL && why == "batch is NULL");
  auto refused = [&](const char* text) {
    const Verdict s = staged(x);
    EXPECT(s.is(BWAGPU_E_INVAL, text));
  };
  for (int32_t* d : {&b.n_reads, &b.n_chains, &b.n_seeds}) {
    Poke<int32_t> p(d, -1);
    refused("negative batch dimension");
  }
  {
    Poke<int64_t> p(&b.seq_bytes, -1);
    refused("negative batch dimension");
  }
  {
    Poke<const int64_t*> p(&b.seq_off, nullptr);
    refused("NULL offset array");
  }
  for (const int32_t** a : {&b.read_chain_off, &b.chain_seed_off}) {
    Poke<const int32_t*> p(a, nullptr);
    refused("NULL offset array");
  }
  for (int i : {0, 3}) {  // each array's first and last entry
    {
      Poke<int64_t> p(b.seq_off + i, b.seq_off[i] + 1);
      refused("seq_off does not span seq_bytes");
    }
    {
      Poke<int32_t> p(b.read_chain_off + i, b.read_chain_off[i] + 1);
      refused("read_chain_off does not span n_chains");
    }
    {
      Poke<int32_t> p(b.chain_seed_off + i, b.chain_seed_off[i] + 1);
      refused("chain_seed_off does not span n_seeds");
    }
  }
  {
    Poke<const int32_t*> p(&b.chain_rid, nullptr);
    refused("NULL chain array");
  }
  {
    Poke<const float*> p(&b.chain_frac_rep, nullptr);
    refused("NULL chain array");
  }
  {
    Poke<const bwagpu_seed_t*> p(&b.seeds, nullptr);
    refused("NULL seeds");
  }
  {
    Poke<const uint8_t*> p(&b.seq, nullptr);
    refused("NULL seq");
  }
  // no reads: accepted, and nothing is read or written (there is nothing to read)
  bwagpu_batch_t e{};
  e.n_chains = 5, e.n_seeds = 7, e.seq_bytes = 9;
  int lq = -1;
  EXPECT(check_batch_header(&e, &why) == BWAGPU_OK);
  InLayout L;
  L.make(e);
  EXPECT(stage_and_check(&e, kLPac, nullptr, L, &lq, &why) == BWAGPU_OK && lq == 0);
  lq = -1;
  EXPECT(check_batch_seeds(&e, kLPac, &lq, &why) == BWAGPU_OK && lq == 0);
}

static void staging_equals_arrays(Batch& x) {
  const bwagpu_batch_t& b = x.b;
  const size_t nr = (size_t)b.n_reads, nc = (size_t)b.n_chains, ns = (size_t)b.n_seeds;
  std::memset(x.h, 0x5a, x.L.total);
  const Verdict s = staged(x);
  EXPECT(s.rc == BWAGPU_OK);
  EXPECT(!std::memcmp(x.h + x.L.seq_off, b.seq_off, sizeof(int64_t) * (nr + 1)));
  EXPECT(!std::memcmp(x.h + x.L.rco, b.read_chain_off, sizeof(int32_t) * (nr + 1)));
  EXPECT(!std::memcmp(x.h + x.L.cso, b.chain_seed_off, sizeof(int32_t) * (nc + 1)));
  EXPECT(!std::memcmp(x.h + x.L.rid, b.chain_rid, sizeof(int32_t) * nc));
  EXPECT(!std::memcmp(x.h + x.L.frac, b.chain_frac_rep, sizeof(float) * nc));
  EXPECT(!std::memcmp(x.h + x.L.seeds, b.seeds, sizeof(bwagpu_seed_t) * ns));
  EXPECT(!std::memcmp(x.h + x.L.seq, b.seq, (size_t)b.seq_bytes));
}

static void batch_cases() {
  header_cases();
  {  // three reads: one thread, one block
    Batch x(3, len_small);
    defects_on_read(x, 1);
    long_read(3, 1);
    staging_equals_arrays(x);
    EXPECT(staged(x).lq == 22 && checked(x).lq == 22);  // reads of 20, 21, 22 bases
  }
  // Threaded: 67,573 seeds (>= 65536) in 66 blocks of 1024 reads, the last one of 1013; stage_and_check's
  // eight threads take blocks [0,8) [8,16) [16,24) [24,33) [33,41) [41,49) [49,57) [57,66), check_batch_seeds'
  // four a quarter of the reads each
  const int nr = 65536 + 2037, last_blk = nr / 1024 * 1024;
  Batch x(nr, [](int r) { return r == 40000 ? 700 : len_small(r); });
  {
    const Verdict s = staged(x);
    EXPECT(s.rc == BWAGPU_OK && s.lq == 700);  // the true maximum: read 40000's
    EXPECT(s == checked(x) && s == sequential(x));
    staging_equals_arrays(x);
  }
  // the first read of a block (and of a thread's range), the last read of a block, the last block
  for (int r : {1024 * 8, 1024 * 17 + 1023, last_blk, last_blk + 500, nr - 2}) defects_on_read(x, r);
  long_read(nr, 1024 * 8);
  long_read(nr, 1024 * 17 + 1023);
  long_read(nr, nr - 1);
  {  // a block's boundary offsets themselves: refused before anything is copied out of that range
    Poke<int32_t> p(x.b.read_chain_off + 1024, x.b.n_chains + 7);
    EXPECT(staged(x).is(BWAGPU_E_INVAL, kRco));
  }
  {
    Poke<int32_t> p(x.b.chain_seed_off + x.b.read_chain_off[2048], -3);
    EXPECT(staged(x).is(BWAGPU_E_INVAL, kCso));
  }
  {
    Poke<int64_t> p(x.b.seq_off + 2048, x.b.seq_bytes + 9);
    EXPECT(staged(x).is(BWAGPU_E_INVAL, kSeqOff));
  }
  {  // the last block's end offsets (header-checked) with a defect just before them
    Poke<int32_t> p(x.b.chain_seed_off + nr - 1, x.b.n_seeds + 1);
    expect_all(x, BWAGPU_E_INVAL, kCso);
  }
  // two defects of different kinds in two threads' ranges: the earlier read's is reported
  const int r1 = 1024 * 20 + 5, r2 = 1024 * 50 + 7;
  {
    Poke<int64_t> p1(x.b.seq_off + r1, x.b.seq_off[r1 + 1] + 1);  // code 1
    Poke<int32_t> p2(&x.b.seeds[r2].qbeg, -1);                    // code 5
    const Verdict q = sequential(x);
    EXPECT(q.is(BWAGPU_E_INVAL, kSeqOff));
    EXPECT(staged(x) == q && checked(x) == q);
  }
  {
    Poke<int32_t> p1(&x.b.seeds[r1].len, 0);           // code 5
    Poke<int32_t> p2(x.b.read_chain_off + r2, -5);     // code 3
    const Verdict q = sequential(x);
    EXPECT(q.is(BWAGPU_E_INVAL, kSeed));
    EXPECT(staged(x) == q && checked(x) == q);
  }
}

// ------------------------------------------------------------------- seeding
static const bwagpu_seedopt_t kSeedOpt = {19, 10, 20, 1.5f};

struct SeedRun {
  int rc = 0, lq = -1;
  int64_t nb = -1;
  std::string why;
  bool is(int code, const char* text) const { return rc == code && why == text; }
};

// the two checks as seeding runs them; copy: into a destination of exactly the bytes the pass may write
static SeedRun seed_run(int32_t n_reads, const int64_t* so, const uint8_t* seq, bool copy) {
  SeedRun v;
  const char* why = "";
  if ((v.rc = seed_batch_check(&kSeedOpt, n_reads, so, seq, &v.nb, &why)) || n_reads == 0) return v.why = why, v;
  const size_t ob = sizeof(int64_t) * ((size_t)n_reads + 1);
  char* dst = copy ? exact<char>(ob + (size_t)v.nb) : nullptr;
  v.rc = seed_reads_check(n_reads, so, seq, v.nb, dst, &v.lq, &why);
  v.why = why;
  if (copy && v.rc == BWAGPU_OK) {
    EXPECT(!std::memcmp(dst, so, ob));
    EXPECT(!std::memcmp(dst + ob, seq, (size_t)v.nb));
  }
  std::free(dst);
  return v;
}

// reads of BWAGPU_MAX_SEED_READ bases and a last shorter one, nb bases in all (nb % 8 != 0: a scalar tail)
static void seed_cases(int64_t nb) {
  const int32_t nr = (int32_t)((nb + BWAGPU_MAX_SEED_READ - 1) / BWAGPU_MAX_SEED_READ);
  int64_t* so = exact<int64_t>((size_t)nr + 1);
  uint8_t* seq = exact<uint8_t>((size_t)nb);
  for (int32_t r = 0; r <= nr; ++r) so[r] = std::min<int64_t>(nb, (int64_t)r * BWAGPU_MAX_SEED_READ);
  for (int64_t i = 0; i < nb; ++i) seq[i] = (uint8_t)((i * 3 + i / 11) % 5);
  for (bool copy : {false, true}) {
    const SeedRun ok = seed_run(nr, so, seq, copy);  // a read of exactly BWAGPU_MAX_SEED_READ is accepted
    EXPECT(ok.rc == BWAGPU_OK && ok.nb == nb && ok.lq == std::min<int64_t>(nb, BWAGPU_MAX_SEED_READ));
  }
  {
    Poke<int64_t> p(so, 1);
    EXPECT(seed_run(nr, so, seq, true).is(BWAGPU_E_INVAL, "seq_off must start at 0"));
  }
  EXPECT(seed_run(nr, so, nullptr, false).is(BWAGPU_E_INVAL, "seq_off must start at 0"));  // bases without seq
  {
    Poke<int64_t> p(so + 1, so[2] + 1);  // read 1 has length -1
    EXPECT(seed_run(nr, so, seq, true).is(BWAGPU_E_INVAL, "seq_off not monotone"));
  }
  {
    Poke<int64_t> p(so + nr / 2, so[nr / 2] - 1);  // read nr / 2 has BWAGPU_MAX_SEED_READ + 1 bases
    EXPECT(seed_run(nr, so, seq, true).is(BWAGPU_E_UNSUPPORTED, "read longer than BWAGPU_MAX_SEED_READ"));
  }
  // a bad base: the first byte, the last (in the scalar tail), and both sides of the boundary between two
  // threads' ranges (thread 3 ends and thread 4 starts at nb * 4 / 8 rounded down to 8)
  const int64_t mid = (nb * 4 / 8) & ~(int64_t)7;
  for (int64_t at : {(int64_t)0, nb - 1, mid - 1, mid})
    for (int v : {5, 0x7f, 0x80, 0xff}) {
      Poke<uint8_t> p(seq + at, (uint8_t)v);
      EXPECT(seed_run(nr, so, seq, v == 5).is(BWAGPU_E_INVAL, "read base > 4 (bases are nt4)"));
    }
  {  // 4 is a base
    Poke<uint8_t> p(seq + nb - 1, 4), q(seq + mid, 4);
    EXPECT(seed_run(nr, so, seq, false).rc == BWAGPU_OK);
  }
  std::free(so);
  std::free(seq);
}

static void seed_option_cases() {
  int64_t nb = -1;
  const char* why = "";
  bwagpu_seedopt_t o = kSeedOpt;
  o.min_seed_len = 0;
  EXPECT(seed_batch_check(&o, 0, nullptr, nullptr, &nb, &why) == BWAGPU_E_INVAL && !std::strcmp(why, "bad seeding options"));
  o = kSeedOpt, o.split_width = -1;
  EXPECT(seed_batch_check(&o, 0, nullptr, nullptr, &nb, &why) == BWAGPU_E_INVAL && !std::strcmp(why, "bad seeding options"));
  EXPECT(seed_batch_check(&kSeedOpt, 0, nullptr, nullptr, &nb, &why) == BWAGPU_OK && nb == 0);  // no reads: nothing read
  {  // a read one base over the limit, alone
    int64_t* so = exact<int64_t>(2);
    uint8_t* seq = exact<uint8_t>(BWAGPU_MAX_SEED_READ + 1);
    std::memset(seq, 2, BWAGPU_MAX_SEED_READ + 1);
    so[0] = 0, so[1] = BWAGPU_MAX_SEED_READ + 1;
    EXPECT(seed_run(1, so, seq, true).is(BWAGPU_E_UNSUPPORTED, "read longer than BWAGPU_MAX_SEED_READ"));
    std::free(so);
    std::free(seq);
  }
  bwagpu_chainopt_t c = {500, 10000, 0, 1 << 30, 0.5f, 0.5f};
  EXPECT(chain_opt_check(&c, &why) == BWAGPU_OK);
  for (int k = 0; k < 5; ++k) {
    bwagpu_chainopt_t d = c;
    if (k == 0) d.max_occ = 0;
    if (k == 1) d.max_chain_gap = -1;
    if (k == 2) d.max_chain_extend = -1;
    if (k == 3) d.mask_level = nanf("");
    if (k == 4) d.drop_ratio = -0.5f;
    EXPECT(chain_opt_check(&d, &why) == BWAGPU_E_INVAL && !std::strcmp(why, "bad chaining options"));
  }
  bwagpu_bwt_t w{};
  w.seq_len = 1000, w.L2[4] = 1000, w.primary = 17, w.bwt_size = 8 * 16, w.sa_intv = 32, w.n_sa = 1000 / 32 + 1;
  EXPECT(bwt_header_check(&w, &why) == BWAGPU_OK && bwt_sa_check(&w, &why) == BWAGPU_OK);
  for (int k = 0; k < 3; ++k) {
    bwagpu_bwt_t d = w;
    if (k == 0) d.bwt_size = 8 * 16 - 1;
    if (k == 1) d.L2[4] = 999;
    if (k == 2) d.primary = 1001;
    EXPECT(bwt_header_check(&d, &why) == BWAGPU_E_INVAL &&
           !std::strcmp(why, "bwt header inconsistent with its occurrence array"));
  }
  for (int k = 0; k < 3; ++k) {
    bwagpu_bwt_t d = w;
    if (k == 0) d.sa_intv = 0;
    if (k == 1) d.sa_intv = 24;
    if (k == 2) d.n_sa = 1000 / 32;
    EXPECT(bwt_sa_check(&d, &why) == BWAGPU_E_INVAL &&
           !std::strcmp(why, "suffix array sample interval / size inconsistent"));
  }
}

// mem_flt_chained_seeds' gate (bwamem.c:576-578, 609-611), transcribed
#define MEM_HSP_COEF 1.1f
#define MEM_MINSC_COEF 5.5f
#define MEM_SEEDSW_COEF 0.05f
static int ref_min_hsp_score(int min_chain_weight, int a, int l_query) {  // -1: the read is not realigned
  double min_l = min_chain_weight ? MEM_HSP_COEF * min_chain_weight : MEM_MINSC_COEF * log(l_query);
  int min_HSP_score = (int)(a * min_l + .499);
  if (min_l > MEM_SEEDSW_COEF * l_query) return -1;
  return min_HSP_score;
}

static void gate_table_cases() {
  const int lq_max = 4096;
  int64_t* so = exact<int64_t>((size_t)lq_max + 1);  // reads of 1 .. 4096 bases
  so[0] = 0;
  for (int l = 1; l <= lq_max; ++l) so[l] = so[l - 1] + l;
  for (int mcw : {0, 3})
    for (int a : {1, 2}) {
      bwagpu_chainopt_t c = {500, 10000, mcw, 1 << 30, 0.5f, 0.5f};
      std::vector<int32_t> tab;
      const bool any = seed_sw_table(&c, a, 19, lq_max, so, lq_max, &tab);
      EXPECT(tab.size() == (size_t)lq_max + 1 && tab[0] == -1 && any);
      int first = 0;  // the shortest realigned length of at least min_seed_len (log(1) = 0 passes the gate too)
      for (int l = 1; l <= lq_max; ++l) {
        EXPECT(tab[(size_t)l] == ref_min_hsp_score(mcw, a, l));
        if (!first && l >= 19 && tab[(size_t)l] >= 0) first = l;
      }
      EXPECT(first > 19 && first < lq_max);
      // any_sw follows min_seed_len and the lengths the batch has
      EXPECT(seed_sw_table(&c, a, lq_max, lq_max, so, lq_max, &tab));       // only the longest read qualifies
      EXPECT(!seed_sw_table(&c, a, lq_max + 1, lq_max, so, lq_max, &tab));  // no read has min_seed_len bases
      EXPECT(!seed_sw_table(&c, a, 19, first - 1, so, first - 1, &tab));    // every read is below the gate
      EXPECT(seed_sw_table(&c, a, 19, first, so, first, &tab));
    }
  std::free(so);
}

// ---------------------------------------------------------------------- pool
static bool pool_sums(int nt) {  // nt disjoint ranges of 0 .. n - 1, each summed by its task
  const int n = 100003;
  std::vector<int64_t> part((size_t)nt, 0);
  host_parallel(nt, [&](int t) {
    int64_t s = 0;
    for (int64_t i = (int64_t)n * t / nt; i < (int64_t)n * (t + 1) / nt; ++i) s += i;
    part[(size_t)t] = s;
  });
  int64_t sum = 0;
  for (int64_t s : part) sum += s;
  return sum == (int64_t)n * (n - 1) / 2;
}

static void pool_cases() {
  for (int nt : {1, 2, 8, 32}) EXPECT(pool_sums(nt));  // 32: more tasks than pool threads
  std::atomic<int> bad{0};  // two callers at once
  auto caller = [&] {
    for (int k = 0; k < 50; ++k)
      for (int nt : {2, 8, 32})
        if (!pool_sums(nt)) ++bad;
  };
  std::thread a(caller), b(caller);
  a.join();
  b.join();
  EXPECT(bad == 0);
  EXPECT(&PassPool::get() == &PassPool::get());
}

int main() {
  pool_cases();
  batch_cases();
  seed_option_cases();
  seed_cases(3 * BWAGPU_MAX_SEED_READ + 5);  // one thread
  seed_cases(((int64_t)1 << 22) + 5);        // eight
  gate_table_cases();
  if (g_fail) {
    std::printf("batch_host_asan: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("batch_host_asan OK\n");
  return 0;
}
