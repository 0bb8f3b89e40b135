// cdn::floor_div_512n (taichi_image_amd/csrc/isp_chroma_denoise.h, the division of the chroma noise filter's db and dr)
// against floor division, for every window count n in 1 .. 49 and every numerator in [-(2^24 + 256 * 49), 2^24 + 256 * 49];
// and cdn::green_delta against the contract's expression for every pair of deltas.  Prints "ok <n>" per divisor, or FAIL
// lines.  Built and run by tests/test_chroma_denoise_cpu.py.
#include <cstdio>

#include "../taichi_image_amd/csrc/isp_chroma_denoise.h"

static long long floor_div(long long a, long long b) {       // b > 0
  long long q = a / b;
  if (a % b != 0 && a < 0) --q;
  return q;
}

int main() {
  const int LIM = (1 << 24) + 256 * 49;
  int bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(dynamic)
  for (int n = 1; n <= 49; ++n) {
    int fails = 0;
    for (int num = -LIM; num <= LIM; ++num) {
      const int got = cdn::floor_div_512n(num, n);
      const long long want = floor_div(num, 512LL * n);
      if (got != want && fails++ < 5) std::printf("FAIL n %d num %d: got %d want %lld\n", n, num, got, want);
    }
    if (!fails) std::printf("ok %d\n", n);
    bad += fails;
  }
  int gfails = 0;
  for (int dr = -256; dr <= 256; ++dr)
    for (int db = -256; db <= 256; ++db) {
      const long long want = floor_div((-(77LL * dr + 29LL * db)) * 437 + 32768, 65536);
      if (cdn::green_delta(dr, db) != want && gfails++ < 5) std::printf("FAIL dg dr %d db %d\n", dr, db);
    }
  if (!gfails) std::printf("green ok\n");
  return bad || gfails ? 1 : 0;
}
