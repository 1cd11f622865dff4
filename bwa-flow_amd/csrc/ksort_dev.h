// ksort_dev.h — klib's introsort (ksort.h:146-226) step for step on the
// device: insertion sort up to 16-element runs, median-of-three partitions,
// comb sort past the depth limit.  It is not stable for n > 17, so a restatement
// must make the same comparisons and the same moves to leave ties in the
// reference's order.  Shared by mem_chain_flt (chain.hip) and the region
// post-processing (regpost.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace bwagpu {

template <class I, class LT>
__device__ void c_insert(I* a, int s, int t, LT lt) {  // [s, t)
  for (int i = s + 1; i < t; ++i)
    for (int j = i; j > s && lt(a[j], a[j - 1]); --j) {
      const auto x = a[j];
      a[j] = a[j - 1];
      a[j - 1] = x;
    }
}
template <class I, class LT>
__device__ void c_comb(I* a, int s, int n, LT lt) {  // a[s, s+n)
  const double shrink = 1.2473309501039786540366528676643;
  int gap = n;
  bool swapped;
  do {
    if (gap > 2) {
      gap = (int)(gap / shrink);
      if (gap == 9 || gap == 10) gap = 11;
    }
    swapped = false;
    for (int i = s; i < s + n - gap; ++i)
      if (lt(a[i + gap], a[i])) {
        const auto x = a[i];
        a[i] = a[i + gap];
        a[i + gap] = x;
        swapped = true;
      }
  } while (swapped || gap > 2);
  if (gap != 1) c_insert(a, s, s + n, lt);
}
template <class I, class LT>
__device__ void c_introsort(int n, I* a, LT lt) {
  if (n < 1) return;
  if (n == 2) {
    if (lt(a[1], a[0])) {
      const auto x = a[0];
      a[0] = a[1];
      a[1] = x;
    }
    return;
  }
  int d = 2;
  while ((1 << d) < n) ++d;
  struct Frame {
    int l, r, d;
  } stack[64];
  int top = 0, s = 0, t = n - 1;
  d <<= 1;
  for (;;) {
    if (s < t) {
      if (--d == 0) {
        c_comb(a, s, t - s + 1, lt);
        t = s;
        continue;
      }
      int i = s, j = t, k = i + ((j - i) >> 1) + 1;
      if (lt(a[k], a[i])) {
        if (lt(a[k], a[j])) k = j;
      } else {
        k = lt(a[j], a[i]) ? i : j;
      }
      const auto rp = a[k];
      if (k != t) {
        a[k] = a[t];
        a[t] = rp;
      }
      for (;;) {
        do ++i; while (lt(a[i], rp));
        do --j; while (i <= j && lt(rp, a[j]));
        if (j <= i) break;
        const auto x = a[i];
        a[i] = a[j];
        a[j] = x;
      }
      {
        const auto x = a[i];
        a[i] = a[t];
        a[t] = x;
      }
      if (i - s > t - i) {
        if (i - s > 16) stack[top++] = Frame{s, i - 1, d};
        s = t - i > 16 ? i + 1 : t;
      } else {
        if (t - i > 16) stack[top++] = Frame{i + 1, t, d};
        t = i - s > 16 ? i - 1 : s;
      }
    } else {
      if (top == 0) {
        c_insert(a, 0, n, lt);
        return;
      }
      --top;
      s = stack[top].l;
      t = stack[top].r;
      d = stack[top].d;
    }
  }
}

}  // namespace bwagpu
