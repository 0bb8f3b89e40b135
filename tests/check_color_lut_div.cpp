// clut::div255 (taichi_image_amd/csrc/isp_color_lut.h, the division of the colour LUT's p_c and of its y_c) against x / 255 for
// every x in 0 .. 65025 + 127, the largest numerator of the contract.  Prints "ok <count>", or FAIL lines.  Built and run by
// tests/test_color_lut_cpu.py.
#include <cstdio>

#include "../taichi_image_amd/csrc/isp_color_lut.h"

int main() {
  int fails = 0;
  const unsigned LIM = 65025u + 127u;
  for (unsigned x = 0; x <= LIM; ++x) {
    const unsigned got = clut::div255(x), want = x / 255u;
    if (got != want && fails++ < 5) std::printf("FAIL x %u: got %u want %u\n", x, got, want);
  }
  if (!fails) std::printf("ok %u\n", LIM + 1);
  return fails ? 1 : 0;
}
