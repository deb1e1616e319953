// shade_consts_check.cpp — stand-alone check (no GPU, no library) that the cheaper forms of the SHADE / GEN turn in csrc/ray_math.h compute
// what the forms they stand in for compute, bit for bit:
//   1. sincos_deg_table_small and sincos_deg_table_turn against sincos_deg_table over EVERY binary32 angle of their domains (|th| <= 2.4
//      with both zeros and all denormals; +0 <= th <= 6.2831855f), and their callers sample_disc_concentric and rng_gauss2 against the
//      forms that call sincos_deg_table, over special uniforms (generator states made to draw them) and a few million draws;
//   2. dielectric() on the material's constants (dielectric_consts) against dielectric() with its two divisions, over indices of
//      refraction {1, 1.52, 0.5, 1e-30, 1e30, 0, inf, NaN, ..} and random ones, special and random directions and normals on both
//      sides of the surface, u1 over 0, 1 and random values: the direction's bits and the returned flag.
// Every output bit is compared, a NaN's bits included - except where an INPUT holds a NaN: such a NaN meets NaNs of the other sign
// (n = -n, cost1 = -ndotr), which of the two a commutative operation then returns is the compiler's operand order, and the forms are
// only asked for a NaN in the same places (diffuse_frame_check.cpp says the same of the frame).
// Exit status 0 and "shade_consts_check OK" = no difference. Built and run by tests/test_shade_consts.py with the library's exact flags.
#include "../ray_math.h"

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

namespace {

using mi::f3;
using mi::mk;

uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
float from_bits(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }

uint64_t rngState = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17; return (uint32_t)(rngState >> 16); }
float rndUnit() { return (float)(rnd() >> 8) * (1.f / 16777216.f); }      // [0, 1)

float sinTbl[92];
std::atomic<long> failures{0};

// ---- 1. bounded sincos ------------------------------------------------------------------------------------------------------------
// bit patterns [lo, hi] (one sign), in `threads` slices
template <class F>
void sweep(uint32_t lo, uint32_t hi, unsigned threads, F&& one) {
  std::vector<std::thread> pool;
  const uint64_t count = (uint64_t)hi - lo + 1u;
  for (unsigned t = 0; t < threads; ++t) {
    const uint32_t a = lo + (uint32_t)(count * t / threads), b = lo + (uint32_t)(count * (t + 1) / threads);      // [a, b)
    pool.emplace_back([a, b, &one]() { for (uint32_t v = a; v != b; ++v) one(from_bits(v)); });
  }
  for (auto& th : pool) th.join();
}
void check_small(float th) {
  float ws, wc, gs, gc;
  mi::sincos_deg_table(th, sinTbl, ws, wc);
  mi::sincos_deg_table_small(th, sinTbl, gs, gc);
  if ((bits(ws) != bits(gs) || bits(wc) != bits(gc)) && failures++ < 10)
    std::printf("sincos_deg_table_small differs for th = %08x: want %08x %08x, got %08x %08x\n", bits(th), bits(ws), bits(wc), bits(gs), bits(gc));
}
void check_turn(float th) {
  float ws, wc, gs, gc;
  mi::sincos_deg_table(th, sinTbl, ws, wc);
  mi::sincos_deg_table_turn(th, sinTbl, gs, gc);
  if ((bits(ws) != bits(gs) || bits(wc) != bits(gc)) && failures++ < 10)
    std::printf("sincos_deg_table_turn differs for th = %08x: want %08x %08x, got %08x %08x\n", bits(th), bits(ws), bits(wc), bits(gs), bits(gc));
}

// the two callers as they stood, on the general form
void disc_general(float u1, float u2, float& ox, float& oy) {
  const float ux = 2.f * u1 - 1.f, uy = 2.f * u2 - 1.f;
  if (ux == 0.f && uy == 0.f) { ox = ux; oy = uy; return; }
  const float piby4 = (float)(3.14159265358979323846264338327950288 / 4.0);
  const float piby2 = (float)(3.14159265358979323846264338327950288 / 2.0);
  const bool wide = fabsf(ux) > fabsf(uy);
  const float r = wide ? ux : uy;
  const float q = piby4 * ((wide ? uy : ux) / (wide ? ux : uy));
  const float th = wide ? q : piby2 - q;
  float s, c;
  mi::sincos_deg_table(th, sinTbl, s, c);
  ox = r * c; oy = r * s;
}
void gauss2_general(mi::Rng& r, float& g0, float& g1) {
  const float ua = mi::rng_uniform01(r);
  const float ub = mi::rng_uniform01(r);
  float w = 1.f - ua;
  if (w < 2.98023223876953125e-08f) w = 2.98023223876953125e-08f;
  const float rad = sqrtf(-2.f * mi::log_det(w));
  float sn, cs;
  mi::sincos_deg_table(6.283185307179586f * ub, sinTbl, sn, cs);
  g0 = rad * cs;
  g1 = rad * sn;
}
void check_disc(float u1, float u2) {
  float wx, wy, gx, gy;
  disc_general(u1, u2, wx, wy);
  mi::sample_disc_concentric(u1, u2, sinTbl, gx, gy);
  if ((bits(wx) != bits(gx) || bits(wy) != bits(gy)) && failures++ < 10)
    std::printf("sample_disc_concentric differs for u = %08x %08x: want %08x %08x, got %08x %08x\n", bits(u1), bits(u2), bits(wx), bits(wy), bits(gx), bits(gy));
}
void check_gauss(mi::Rng r) {
  mi::Rng ra = r, rb = r;
  float w0, w1, g0, g1;
  gauss2_general(ra, w0, w1);
  mi::rng_gauss2(rb, sinTbl, g0, g1);
  if ((bits(w0) != bits(g0) || bits(w1) != bits(g1) || ra.s0 != rb.s0 || ra.s1 != rb.s1) && failures++ < 10)
    std::printf("rng_gauss2 differs for state %016llx %016llx: want %08x %08x, got %08x %08x\n", (unsigned long long)r.s0, (unsigned long long)r.s1, bits(w0), bits(w1), bits(g0), bits(g1));
}
// A generator state whose next two rng_uniform01 draws are ua and ub (values of [0, 1] with 1 + u exact in binary64; 1.0f is drawn as
// the largest mantissa, which narrows to it): xoroshiro128**'s output scrambler and state step are both invertible.
uint64_t draw_for(float u) {
  if (u >= 1.f) return ~0ull << 12;
  const double d = 1.0 + (double)u;
  uint64_t b; std::memcpy(&b, &d, 8);
  return (b & ((1ull << 52) - 1ull)) << 12;
}
uint64_t state_for(uint64_t out) {      // s0 with rotl64(s0 * 5, 7) * 9 == out
  const uint64_t x = out * 0x8E38E38E38E38E39ull;      // 9^-1 mod 2^64
  return ((x >> 7) | (x << 57)) * 0xCCCCCCCCCCCCCCCDull;      // 5^-1
}
mi::Rng rng_drawing(float ua, float ub) {
  mi::Rng r;
  r.s0 = state_for(draw_for(ua));
  const uint64_t f = state_for(draw_for(ub)) ^ mi::rotl64(r.s0, 24);      // = b ^ (b << 16), b = s1 ^ s0
  const uint64_t b = f ^ (f << 16) ^ (f << 32) ^ (f << 48);
  r.s1 = b ^ r.s0;
  return r;
}

// ---- 2. the dielectric bounce -------------------------------------------------------------------------------------------------------
bool any_nan(f3 v) { return std::isnan(v.x) || std::isnan(v.y) || std::isnan(v.z); }
bool same_dir(f3 w, f3 g, bool nanInput) {
  const uint32_t a[3] = {bits(w.x), bits(w.y), bits(w.z)}, b[3] = {bits(g.x), bits(g.y), bits(g.z)};
  for (int k = 0; k < 3; ++k) {
    if (a[k] == b[k]) continue;
    if (nanInput && std::isnan(from_bits(a[k])) && std::isnan(from_bits(b[k]))) continue;
    return false;
  }
  return true;
}
void report(const char* what, f3 d, f3 n, float ior, float u1, f3 w, bool wf, f3 g, bool gf) {
  if (failures++ < 10)
    std::printf("%s differs for d = %08x %08x %08x, n = %08x %08x %08x, ior = %08x, u1 = %08x: want %08x %08x %08x (%d), got %08x %08x %08x (%d)\n", what, bits(d.x), bits(d.y), bits(d.z),
                bits(n.x), bits(n.y), bits(n.z), bits(ior), bits(u1), bits(w.x), bits(w.y), bits(w.z), (int)wf, bits(g.x), bits(g.y), bits(g.z), (int)gf);
}
long bounces = 0;
void check_bounce(f3 d, f3 n, float ior, float u1) {
  const bool nanInput = any_nan(d) || any_nan(n) || std::isnan(ior) || std::isnan(u1);
  const mi::DielectricConsts k = mi::dielectric_consts(ior);
  f3 w, g;
  const bool wf = mi::dielectric(d, n, ior, u1, w);
  bool gf = mi::dielectric(d, n, ior, k, u1, g);
  if (gf != wf || !same_dir(w, g, nanInput)) report("dielectric on constants", d, n, ior, u1, w, wf, g, gf);
  gf = mi::dielectric_with(d, n, ior, mi::DielectricComputed{}, u1, g);      // (K1w's form where the materials are not staged)
  if (gf != wf || !same_dir(w, g, nanInput)) report("dielectric_with, computed ratio", d, n, ior, u1, w, wf, g, gf);
  ++bounces;
}

}  // namespace

int main() {
  { static const uint32_t tblBits[92] = {MI_SIN_TABLE_BITS}; std::memcpy(sinTbl, tblBits, sizeof sinTbl); }
  unsigned threads = std::thread::hardware_concurrency();
  threads = threads < 1u ? 1u : threads > 16u ? 16u : threads;

  // ---- every angle of the two domains ----
  const uint32_t smallTop = bits(2.4f), turnTop = bits(6.2831855f);
  sweep(0u, smallTop, threads, check_small);                                // +0, the denormals, .. 2.4
  sweep(0x80000000u, 0x80000000u | smallTop, threads, check_small);         // -0 .. -2.4
  sweep(0u, turnTop, threads, check_turn);
  const unsigned long long angles = 2ull * ((unsigned long long)smallTop + 1u) + turnTop + 1u;

  // ---- the two callers ----
  const float half = 0.5f, one = 1.f;
  const std::vector<float> us = {0.f, half, one, from_bits(bits(half) - 1u), from_bits(bits(half) + 1u), from_bits(bits(half) - 2u), from_bits(bits(half) + 2u), 0.25f, 0.75f,
                                 from_bits(bits(one) - 1u), from_bits(bits(one) - 2u), from_bits(0x33800000u), from_bits(0x34000000u), 0.125f, 0.875f, 0.1f, 0.9f, 1e-10f};
  long discs = 0, gausses = 0;
  for (float a : us) for (float b : us) { check_disc(a, b); ++discs; }
  for (int k = 0; k < 2000000; ++k) {
    const float a = rndUnit(), m = 1.f - a;
    for (float b : {a, m, from_bits(bits(a) + 1u), from_bits(bits(m) + 1u), rndUnit(), half, 0.f, one}) { check_disc(a, b); check_disc(b, a); discs += 2; }
  }
  // (the uniforms a state can be made to draw: 1 + u exact in binary64; 0.1f, 0.9f and the like are)
  for (float a : us) for (float b : us) {
    if (a == 1e-10f || b == 1e-10f) continue;
    mi::Rng r = rng_drawing(a, b), probe = r;
    const float da = mi::rng_uniform01(probe), db = mi::rng_uniform01(probe);
    if ((bits(da) != bits(a) || bits(db) != bits(b)) && failures++ < 10) std::printf("the check's own state for draws %08x %08x draws %08x %08x\n", bits(a), bits(b), bits(da), bits(db));
    check_gauss(r); ++gausses;
  }
  for (int k = 0; k < 4000000; ++k) {
    mi::Rng r;
    r.s0 = ((uint64_t)rnd() << 32) | rnd(); r.s1 = ((uint64_t)rnd() << 32) | rnd();
    if (k & 1) r = rng_drawing(rndUnit(), (k & 2) ? from_bits(bits(one) - 1u - (rnd() & 7u)) : rndUnit());      // (angles next to the full turn)
    check_gauss(r); ++gausses;
  }

  // ---- the bounces ----
  const float inf = INFINITY, qnan = from_bits(0x7FC00000u), nnan = from_bits(0xFFC00001u);
  const float iors[] = {1.f, 1.52f, 0.5f, 1e-30f, 1e30f, 0.f, inf, qnan, 1.33f, 2.4f, -1.5f};
  const float u1s[] = {0.f, 1.f, 0.5f, 0.04f, from_bits(bits(one) - 1u), from_bits(0x33800000u)};
  const float comps[] = {0.f, -0.f, 1.f, -1.f, 0.70710678f, -0.70710678f, 0.6f, -0.8f, from_bits(1u), 1e-30f, -1e-20f, 1e19f, 3e38f, inf, -inf, qnan, nnan};
  std::vector<f3> vs;
  for (float x : comps) for (float y : comps) for (float z : comps) {
    const int odd = (std::isfinite(x) && fabsf(x) <= 1.f ? 0 : 1) + (std::isfinite(y) && fabsf(y) <= 1.f ? 0 : 1) + (std::isfinite(z) && fabsf(z) <= 1.f ? 0 : 1);
    if (odd <= 1) vs.push_back(mk(x, y, z));      // (at most one component that no direction has: the pairs below are many enough)
  }
  for (size_t i = 0; i < vs.size(); ++i)
    for (size_t j = i % 7; j < vs.size(); j += 7)
      check_bounce(vs[i], vs[j], iors[(i + j) % 11], u1s[(i + 3 * j) % 6]);
  for (int k = 0; k < 3000000; ++k) {
    const f3 d = mi::normalized(mk(rndUnit() * 2.f - 1.f, rndUnit() * 2.f - 1.f, rndUnit() * 2.f - 1.f));
    f3 n = mi::normalized(mk(rndUnit() * 2.f - 1.f, rndUnit() * 2.f - 1.f, rndUnit() * 2.f - 1.f));
    if (k % 16 == 0) n = (k & 16) ? d : -d;                                              // normal incidence, either side
    if (k % 16 == 1) n = mi::normalized(mi::cross(d, n));                                // grazing
    const float ior = (k % 3 == 0) ? iors[k % 11] : (k % 3 == 1) ? 0.25f + 3.f * rndUnit() : from_bits(rnd());
    const float u1 = (k % 5 == 0) ? u1s[k % 6] : rndUnit();
    check_bounce(d, n, ior, u1);
    check_bounce(d, -n, ior, u1);                                                        // the other side of the surface
  }
  for (int k = 0; k < 500000; ++k)
    check_bounce(mk(from_bits(rnd()), from_bits(rnd()), from_bits(rnd())), mk(from_bits(rnd()), from_bits(rnd()), from_bits(rnd())), from_bits(rnd()), (k & 1) ? rndUnit() : from_bits(rnd()));

  if (failures) { std::printf("shade_consts_check FAILED: %ld differences\n", failures.load()); return 1; }
  std::printf("shade_consts_check OK: %llu angles, %ld disc samples, %ld gauss pairs, %ld bounces, all bits equal\n", angles, discs, gausses, bounces);
  return 0;
}
