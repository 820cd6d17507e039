// RzAcc::pack() (csrc/kernels_resize.hip) against its specification, min(255, max(0, (int)c >> 22)) per channel, for every one of the
// 2^32 accumulator values in every byte position.  pack() is written as a clamp of the sum and then the shift, which
// keeps gfx950's v_ashr_pk_u8_i32 out of the kernels; this shows that the rewrite changes no byte.  The kernel file compiles as it is
// over the stand-in for the HIP runtime header (tests/cpp/hip_host_shim).  The four channels of one pack() hold four different values
// (the counter plus a multiple of an odd constant), so every position sees every value once and a channel that leaked into its
// neighbour would show.  The loop reads no memory.
// Built and run by tests/test_resize_pack.py:  g++ -O2 -std=c++20 -x c++ -Itests/cpp/hip_host_shim ... -pthread
#include <stdio.h>

#include "../../panorama-opticalflow_amd/csrc/kernels_resize.hip"

using namespace pf;

static inline uint32_t spec(uint32_t c) { return (uint32_t)std::min(255, std::max(0, (int)c >> kRzPrecBits)); }

// the 2^16 values that share their upper half: a plain counted loop, so that the compiler may vectorise it
static void block(uint32_t hi, unsigned long long* bad, unsigned long long* sum, uint32_t* first_bad) {
  const uint32_t step[4] = {0u, 0x9E3779B1u, 0x3C6EF362u, 0xDAA66D13u};
  uint32_t wrong = 0, bytes = 0;
  for (int lo = 0; lo < 65536; ++lo) {
    const uint32_t v = (hi << 16) | (uint32_t)lo;
    RzAcc acc;
    uint32_t want = 0;
    for (int i = 0; i < 4; ++i) { acc.c[i] = v + step[i]; want |= spec(acc.c[i]) << (8 * i); }
    const uint32_t got = acc.pack();
    wrong += got != want;
    bytes += got & 0xffu;
  }
  if (wrong && !*bad) *first_bad = hi << 16;
  *bad += wrong; *sum += bytes;
}

int main() {
  const unsigned n_threads = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  std::vector<unsigned long long> bads(n_threads, 0), sums(n_threads, 0);
  std::vector<uint32_t> firsts(n_threads, 0);
  std::vector<std::thread> threads;
  for (unsigned t = 0; t < n_threads; ++t)
    threads.emplace_back([&, t]() { for (uint32_t hi = t; hi < 65536u; hi += n_threads) block(hi, &bads[t], &sums[t], &firsts[t]); });
  for (auto& th : threads) th.join();
  unsigned long long bad = 0, sum = 0;
  uint32_t first_bad = 0;
  for (unsigned t = 0; t < n_threads; ++t) { if (bads[t] && !bad) first_bad = firsts[t]; bad += bads[t]; sum += sums[t]; }
  // position 0 sees every value once: 2^22 values give each byte 1 .. 254, and 2^31 - 255 * 2^22 give 255
  const unsigned long long want_sum = (1ull << 22) * (254ull * 255 / 2) + ((1ull << 31) - (255ull << 22)) * 255;
  if (bad || sum != want_sum) {
    printf("FAIL: %llu of 2^32 accumulator sets pack to other bytes than the specification's (first in the 65536 from 0x%08x); byte sum %llu, expected %llu\n", bad, first_bad, sum, want_sum);
    return 1;
  }
  printf("ok 4294967296\n");
  return 0;
}
