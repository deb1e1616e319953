// rotl_halves_check.cpp — rotl64 on the two 32-bit halves (csrc/ray_math.h) against the plain 64-bit form, and rng_next over it against a
// copy of the generator on the plain form. A stand-alone program (tests/test_rng_halves.py builds and runs it, once more under
// -fsanitize=address,undefined); no GPU, no library.
//   1. rotl64(x, k) == (x << k) | (x >> (64 - k)) for the generator's three counts k = 7, 24, 37 (24: the halves as they lie; 37: the halves
//      swapped) on 0, all ones, the single bits 0, 31, 32 and 63, values whose halves are equal, and 10^7 random 64-bit values.
//   2. 10^6 draws of rng_next from the seeds 0, 1 and 1442: every output and both state words equal the plain generator's.
// The host's alignbit is the expression the device's v_alignbit_b32 computes ((a : b) >> s, low word; s taken modulo 32 by the
// instruction, and 32 - k lies in 1 .. 31 for these counts), so the one text of rotl64 is what both sides run.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../ray_math.h"

static uint64_t plain_rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
// xoroshiro128** as ray_math.h had it before the halves form
static uint64_t plain_next(mi::Rng& r) {
  const uint64_t a = r.s0;
  uint64_t b = r.s1;
  const uint64_t out = plain_rotl(a * 5, 7) * 9;
  b ^= a;
  r.s0 = plain_rotl(a, 24) ^ b ^ (b << 16);
  r.s1 = plain_rotl(b, 37);
  return out;
}

static unsigned long long bad = 0, cases = 0;
template <int K> static void one(uint64_t x) {
  const uint64_t got = mi::rotl64(x, K), want = plain_rotl(x, K);
  ++cases;
  if (got != want && bad++ < 8) printf("rotl64(%016llx, %d) = %016llx, plain form %016llx\n", (unsigned long long)x, K, (unsigned long long)got, (unsigned long long)want);
}
static void all_counts(uint64_t x) { one<7>(x); one<24>(x); one<37>(x); }

int main() {
  all_counts(0ull);
  all_counts(~0ull);
  for (int bit : {0, 31, 32, 63}) { all_counts(1ull << bit); all_counts(~(1ull << bit)); }
  uint64_t z = 0x243f6a8885a308d3ull;
  for (int i = 0; i < 1000; ++i) { z = mi::splitmix64(z); const uint64_t h = z >> 32; all_counts((h << 32) | h); }      // the two halves equal
  for (int i = 0; i < 10000000; ++i) { z = mi::splitmix64(z); all_counts(z); }
  const unsigned long long rotCases = cases;

  unsigned long long draws = 0;
  for (uint64_t seed : {0ull, 1ull, 1442ull}) {
    mi::Rng a, b;
    mi::rng_seed(a, seed);
    b = a;
    for (int i = 0; i < 1000000; ++i) {
      const uint64_t got = mi::rng_next(a), want = plain_next(b);
      ++draws;
      if ((got != want || a.s0 != b.s0 || a.s1 != b.s1) && bad++ < 8)
        printf("seed %llu draw %d: %016llx state %016llx %016llx, plain generator %016llx state %016llx %016llx\n", (unsigned long long)seed, i, (unsigned long long)got,
               (unsigned long long)a.s0, (unsigned long long)a.s1, (unsigned long long)want, (unsigned long long)b.s0, (unsigned long long)b.s1);
    }
  }
  printf("rotations compared %llu, draws compared %llu, differences %llu\n", rotCases, draws, bad);
  if (bad) return 1;
  printf("rotl_halves_check OK\n");
  return 0;
}
