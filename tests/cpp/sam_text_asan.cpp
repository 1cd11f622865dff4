// The plain-C++ arithmetic of bwagpu_sam_text_device (bwa-flow_amd/csrc/pure.h) as a
// stand-alone program under AddressSanitizer and UBSan, on the CPU: decimal widths
// and digits and the pa:f rounding against snprintf, and the flag, TLEN and clip
// rules against the reference's expressions (bwa/bwamem.c:824-912) restated here.
#include <inttypes.h>
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "pure.h"

using namespace bwagpu;

static int fails = 0;
#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c)) {                            \
      if (++fails < 20) printf(__VA_ARGS__); \
    }                                      \
  } while (0)

static void check_width(int64_t v) {
  char buf[32], mine[32];
  const int w = snprintf(buf, sizeof buf, "%" PRId64, v);
  CHECK(dec_width(v) == w, "width of %" PRId64 ": %d != %d\n", v, dec_width(v), w);
  int at = 0;
  if (v < 0) mine[at++] = '-';
  const int nd = w - (v < 0);
  for (int k = nd - 1; k >= 0; --k) mine[at++] = (char)('0' + dec_digit(dec_mag(v), k));
  mine[at] = 0;
  CHECK(strcmp(buf, mine) == 0, "digits of %" PRId64 ": %s != %s\n", v, mine, buf);
}

static void widths() {
  uint64_t p = 1;
  for (int k = 0; k < 19; ++k, p *= 10) {
    for (int d = -1; d <= 1; ++d) {
      check_width((int64_t)p + d);
      check_width(-((int64_t)p + d));
    }
    if (p <= 1000000000ull) {
      check_width((int32_t)(p - 1));
      check_width(-(int32_t)(p - 1));
    }
  }
  const int64_t ends[] = {0, INT32_MAX, INT32_MIN, (int64_t)INT32_MAX + 1, (int64_t)INT32_MIN - 1, INT64_MAX, INT64_MIN,
                          INT64_MAX - 1, INT64_MIN + 1, 4294967295ll, 4294967296ll, 4999999999ll};
  for (int64_t v : ends) check_width(v);
  char buf[32];
  snprintf(buf, sizeof buf, "%" PRIu64, UINT64_MAX);
  CHECK(dec_width_u64(UINT64_MAX) == (int)strlen(buf), "width of UINT64_MAX\n");
}

static void pa() {
  long differ_from_floor = 0;
  for (int sc = 1; sc <= 1023; ++sc)
    for (int al = 1; al <= 1023; ++al) {
      char want[64], got[64];
      snprintf(want, sizeof want, "%.3f", (double)sc / al);
      bool neg;
      const uint64_t th = pa_thousandths(sc, al, &neg);
      snprintf(got, sizeof got, "%s%" PRIu64 ".%03d", neg ? "-" : "", th / 1000, (int)(th % 1000));
      CHECK(strcmp(want, got) == 0, "pa %d / %d: %s != %s\n", sc, al, got, want);
      if (sc <= 300 && al <= 300) {
        const uint64_t naive = (uint64_t)((double)sc / al * 1000 + .5);
        differ_from_floor += naive != th;
      }
    }
  CHECK(differ_from_floor == 378, "floor(x * 1000 + .5) differs for %ld pairs in 1..300, not 378\n", differ_from_floor);
  const int edge[][2] = {{65, 80}, {1, 16}, {0, 5}, {-1, 10000}, {-65, 80}, {INT32_MAX, 1}, {1, INT32_MAX}, {INT32_MIN, 3},
                         {3, 2048}, {1, 2000}, {-1, 2000}};
  for (auto& e : edge) {
    char want[64], got[64];
    snprintf(want, sizeof want, "%.3f", (double)e[0] / e[1]);
    bool neg;
    const uint64_t th = pa_thousandths(e[0], e[1], &neg);
    snprintf(got, sizeof got, "%s%" PRIu64 ".%03d", neg ? "-" : "", th / 1000, (int)(th % 1000));
    CHECK(strcmp(want, got) == 0, "pa %d / %d: %s != %s\n", e[0], e[1], got, want);
  }
  bool neg;
  CHECK(pa_thousandths(65, 80, &neg) == 812 && pa_thousandths(1, 16, &neg) == 62, "65/80 and 1/16\n");
}

// bwamem.c:844-852 on the reference's own field names
struct Aln {
  int64_t pos;
  int rid, flag, is_rev, n_cigar;
};
static void ref_flags(Aln* p, Aln* m) {
  p->flag |= m ? 0x1 : 0;
  p->flag |= p->rid < 0 ? 0x4 : 0;
  p->flag |= m && m->rid < 0 ? 0x8 : 0;
  if (p->rid < 0 && m && m->rid >= 0) p->rid = m->rid, p->pos = m->pos, p->is_rev = m->is_rev, p->n_cigar = 0;
  if (m && m->rid < 0 && p->rid >= 0) m->rid = p->rid, m->pos = p->pos, m->is_rev = p->is_rev, m->n_cigar = 0;
  p->flag |= p->is_rev ? 0x10 : 0;
  p->flag |= m && m->is_rev ? 0x20 : 0;
}

static void flags_and_tlen() {
  const int rids[] = {-1, 0, 3};
  const int64_t poss[] = {0, 99, 4999999999ll};
  for (int pr : rids)
    for (int mr : rids)
      for (int prev = 0; prev < 2; ++prev)
        for (int mrev = 0; mrev < 2; ++mrev)
          for (int64_t pp : poss)
            for (int64_t mp : poss)
              for (int pn = 0; pn < 3; pn += 2)
                for (int mn = 0; mn < 3; mn += 2)
                  for (int f0 : {0x41, 0x881, 0x43}) {
                    Aln p{pr < 0 ? -1 : pp, pr, f0 | (pr < 0 ? 4 : 0), pr < 0 ? 0 : prev, pr < 0 ? 0 : pn};
                    Aln m{mr < 0 ? -1 : mp, mr, 0, mr < 0 ? 0 : mrev, mr < 0 ? 0 : mn};
                    SamCoord pc{p.pos, p.rid, p.is_rev, p.n_cigar}, mc{m.pos, m.rid, m.is_rev, m.n_cigar};
                    const int flag = sam_flag(p.flag, &pc, &mc);
                    ref_flags(&p, &m);
                    CHECK(flag == p.flag && pc.pos == p.pos && pc.rid == p.rid && pc.is_rev == p.is_rev &&
                              pc.n_cigar == p.n_cigar && mc.pos == m.pos && mc.rid == m.rid && mc.is_rev == m.is_rev &&
                              mc.n_cigar == m.n_cigar,
                          "flags p %d m %d\n", pr, mr);
                    if (p.rid >= 0 && p.rid == m.rid)
                      for (int prl : {1, 150})
                        for (int mrl : {1, 151}) {
                          // bwamem.c:874-877
                          const int64_t p0 = p.pos + (p.is_rev ? prl - 1 : 0);
                          const int64_t p1 = m.pos + (m.is_rev ? mrl - 1 : 0);
                          const int64_t want =
                              (m.n_cigar == 0 || p.n_cigar == 0) ? 0 : -(p0 - p1 + (p0 > p1 ? 1 : p0 < p1 ? -1 : 0));
                          CHECK(sam_tlen(pc, prl, mc, mrl) == want, "tlen\n");
                        }
                  }
}

static void clips() {
  const uint32_t ops[] = {10u << 4 | 3, 7u << 4 | 4, 30u << 4 | 0, 5u << 4 | 1, 2u << 4 | 2};
  for (int opt_flag : {0, 0x200, 0x2000, 0x2200})
    for (int is_alt = 0; is_alt < 2; ++is_alt)
      for (int which = 0; which < 3; ++which) {
        for (int c = 0; c < 5; ++c) {  // add_cigar, bwamem.c:829-831
          int want = c;
          if (!(opt_flag & 0x200) && !is_alt && (c == 3 || c == 4)) want = which ? 4 : 3;
          CHECK(sam_cigar_op(c, sam_clip_rewrite(opt_flag, is_alt), which) == want, "cigar op\n");
        }
        for (uint32_t first : ops)
          for (uint32_t last : ops)
            for (int is_rev = 0; is_rev < 2; ++is_rev) {
              const int l_seq = 100;
              int qb = 0, qe = l_seq;  // bwamem.c:886-890, 900-904 with n_cigar > 0
              if (which && !(opt_flag & 0x200) && !is_alt) {
                const bool c0 = (first & 0xf) == 4 || (first & 0xf) == 3, c1 = (last & 0xf) == 4 || (last & 0xf) == 3;
                if (!is_rev) {
                  if (c0) qb += first >> 4;
                  if (c1) qe -= last >> 4;
                } else {
                  if (c0) qe -= first >> 4;
                  if (c1) qb += last >> 4;
                }
              }
              int gb, ge;
              sam_seq_range(l_seq, which && sam_clip_rewrite(opt_flag, is_alt), is_rev, first, last, &gb, &ge);
              CHECK(gb == qb && ge == qe, "seq range\n");
            }
      }
}

int main() {
  widths();
  pa();
  flags_and_tlen();
  clips();
  if (fails) {
    printf("sam_text_asan: %d failures\n", fails);
    return 1;
  }
  printf("sam_text_asan OK\n");
  return 0;
}
