// side_sort.h — the key order of the phased extension's side lists (spec_side.hip;
// DESIGN.md §27).  Plain C++, host and device in the way pure.h is: compiles
// without HIP.
//
// A side list is sorted by its side's query length, longest first, over 256
// keys.  A key's first position is the exclusive prefix of the list's key
// histogram.  A wave takes the 256 keys four per lane: a lane sums its own four
// counts, the wave scans the 64 lane totals (six shuffle steps on the device,
// side_wave_scan here), and the lane adds what lies before it to its keys.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BWAGPU_SS_HD __host__ __device__
#else
#define BWAGPU_SS_HD
#endif

namespace bwagpu {

constexpr int kSideKeys = 256;
constexpr int kSideLaneKeys = 4;  // keys per lane of a 64-lane wave

BWAGPU_SS_HD inline int side_key(int qlen) { return 255 - (qlen < 255 ? qlen : 255); }  // descending

// a lane's four counts h (keys 4 lane .. 4 lane + 3): their sum
BWAGPU_SS_HD inline int32_t side_lane_total(const int32_t* h) { return h[0] + h[1] + h[2] + h[3]; }
// ... and the keys' first positions, `before` being the sum of every lower lane's counts
BWAGPU_SS_HD inline void side_lane_prefix(const int32_t* h, int32_t before, int32_t* first) {
  first[0] = before;
  first[1] = before + h[0];
  first[2] = first[1] + h[1];
  first[3] = first[2] + h[2];
}
// one step of the wave's inclusive scan: the lane adds the value d lanes below it
BWAGPU_SS_HD inline int32_t side_scan_step(int32_t own, int32_t below, int lane, int d) {
  return lane >= d ? own + below : own;
}

// the 64 lane totals -> their inclusive scan, by the wave's steps (d = 1, 2, .. 32)
BWAGPU_SS_HD inline void side_wave_scan(int32_t* inc) {
  for (int d = 1; d < 64; d <<= 1) {
    int32_t prev[64];
    for (int l = 0; l < 64; ++l) prev[l] = inc[l];
    for (int l = 0; l < 64; ++l) inc[l] = side_scan_step(prev[l], l >= d ? prev[l - d] : 0, l, d);
  }
}
// hist[256] -> first[256]: every key's first position in its list
BWAGPU_SS_HD inline void side_prefix(const int32_t* hist, int32_t* first) {
  int32_t inc[64];
  for (int l = 0; l < 64; ++l) inc[l] = side_lane_total(hist + kSideLaneKeys * l);
  side_wave_scan(inc);
  for (int l = 0; l < 64; ++l)
    side_lane_prefix(hist + kSideLaneKeys * l, inc[l] - side_lane_total(hist + kSideLaneKeys * l),
                     first + kSideLaneKeys * l);
}
// the first position of the list's short run, the sides with a query of up to
// short_q bases (= the sides with a longer query: the list is in descending
// length order)
BWAGPU_SS_HD inline int32_t side_short_first(const int32_t* first, int short_q) { return first[side_key(short_q)]; }

}  // namespace bwagpu
