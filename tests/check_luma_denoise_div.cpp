// ydn::mean_ties_up_rcp (taichi_image_amd/csrc/isp_luma_denoise.h, the division of the luma noise filter's mean) against
// floor((2 s + n) / (2 n)) in integers, for every count n in 1 .. 49, every sum s in 0 .. 255 n and every reciprocal within
// 4 ulp of the host's 1 / n (the device's v_rcp_f32 is within 1 ulp of it); ydn::mean_ties_up likewise; ydn::threshold_at
// against floor division by 256 for every t0, t1 and luma.  Prints "ok <n>" per count, "mean ok", "threshold ok", or FAIL
// lines.  Built and run by tests/test_luma_denoise_cpu.py.
#include <cmath>
#include <cstdio>

#include "../taichi_image_amd/csrc/isp_luma_denoise.h"

static long long floor_div(long long a, long long b) {       // b > 0
  long long q = a / b;
  if (a % b != 0 && a < 0) --q;
  return q;
}

int main() {
  int bad = 0;
  for (int n = 1; n <= 49; ++n) {
    int fails = 0;
    float lo = 1.0f / (float)n, hi = lo;
    for (int k = 0; k < 4; ++k) { lo = std::nextafterf(lo, 0.0f); hi = std::nextafterf(hi, 2.0f); }
    for (float rcp = lo; rcp <= hi; rcp = std::nextafterf(rcp, 2.0f))
      for (int s = 0; s <= 255 * n; ++s) {
        const int got = ydn::mean_ties_up_rcp(s, n, rcp), want = (2 * s + n) / (2 * n);
        if (got != want && fails++ < 5) std::printf("FAIL n %d s %d rcp %a: got %d want %d\n", n, s, rcp, got, want);
      }
    if (!fails) std::printf("ok %d\n", n);
    bad += fails;
  }
  int mfails = 0;
  for (int n = 1; n <= 49; ++n)
    for (int s = 0; s <= 255 * n; ++s) {
      const int want = (2 * s + n) / (2 * n);
      if (ydn::mean_ties_up(s, n) != want && mfails++ < 5) std::printf("FAIL mean n %d s %d\n", n, s);
    }
  if (!mfails) std::printf("mean ok\n");
  int tfails = 0;
  for (int t0 = 0; t0 <= 255; ++t0)
    for (int t1 = 0; t1 <= 255; ++t1)
      for (int L = 0; L <= 255; ++L) {
        const long long want = t0 + floor_div((long long)(t1 - t0) * L + 128, 256);
        const int got = ydn::threshold_at(t0, t1, L);
        if ((got != want || got < 0 || got > 255) && tfails++ < 5) std::printf("FAIL threshold %d %d %d: %d\n", t0, t1, L, got);
      }
  if (!tfails) std::printf("threshold ok\n");
  return bad || mfails || tfails ? 1 : 0;
}
