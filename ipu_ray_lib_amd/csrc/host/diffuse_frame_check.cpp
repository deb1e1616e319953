// diffuse_frame_check.cpp — stand-alone check (no GPU, no library) of the two select forms in csrc/ray_math.h against the branch forms
// they replaced: diffuse_frame (the tangent frame of a diffuse bounce: one sqrt and one division behind selects) and
// sample_disc_concentric (one division behind selects). The branch forms are spelled out below as they stood; every output is compared
// bit for bit, NaN bits included (but see same_bits for a normal that itself holds a NaN), over normals of +-0, denormals, +-inf, NaN, the axis directions, |n.x| == |n.y| ties and a few million
// random unit vectors, and over u in {0, 0.5, 1, neighbours of 0.5, |ux| == |uy|, random}.
// Exit status 0 and "diffuse_frame_check OK" = no difference. Built and run by tests/test_leaf_frame.py with the library's exact flags.
#include "../ray_math.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

using mi::f3;
using mi::mk;

uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
float from_bits(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }

// the reference's two branches, as sample_diffuse carried them
void frame_branches(f3 n, f3& xb, f3& yb) {
  const f3 a = mi::abs3(n), sq = n * n;
  if (a.x > a.y) { const float il = 1.f / sqrtf(sq.x + sq.z); xb = mk(-n.z * il, 0.f, n.x * il); }
  else { const float il = 1.f / sqrtf(sq.y + sq.z); xb = mk(0.f, n.z * il, -n.y * il); }
  yb = mi::cross(n, xb);
}

// the concentric map's angle and radius as its two branches computed them (the sincos that follows is shared)
bool disc_branches(float u1, float u2, float& r, float& th) {
  const float ux = 2.f * u1 - 1.f, uy = 2.f * u2 - 1.f;
  if (ux == 0.f && uy == 0.f) { r = ux; th = uy; return false; }
  const float piby4 = (float)(3.14159265358979323846264338327950288 / 4.0);
  const float piby2 = (float)(3.14159265358979323846264338327950288 / 2.0);
  if (fabsf(ux) > fabsf(uy)) { r = ux; th = piby4 * (uy / ux); }
  else { r = uy; th = piby2 - piby4 * (ux / uy); }
  return true;
}
void disc_reference(float u1, float u2, const float* sinTbl, float& ox, float& oy) {
  float r, th;
  if (!disc_branches(u1, u2, r, th)) { ox = r; oy = th; return; }
  float s, c;
  mi::sincos_deg_table(th, sinTbl, s, c);
  ox = r * c; oy = r * s;
}

uint64_t rngState = 0x9e3779b97f4a7c15ull;
uint32_t rnd() { rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17; return (uint32_t)(rngState >> 16); }
float rndUnit() { return (float)(rnd() >> 8) * (1.f / 16777216.f); }      // [0, 1)

long failures = 0;

// A normal WITHOUT a NaN component: all bits, the bits of every NaN the frame then holds included (those are made by 0 * inf, inf - inf,
// 0 / 0 alone and travel through operations with one NaN operand: defined bits). A normal WITH a NaN component multiplies two NaNs
// of different sign - (-n.y) * il, where il carries n.y's own NaN through square, sum, sqrt and division -, and which operand's bits such a
// product returns is the instruction's operand order, the compiler's choice for a commutative operation: the branch form's own bits
// change with its register allocation. There the frame must hold a NaN exactly where the branch form's does, all other bits equal.
bool same_bits(const uint32_t* w, const uint32_t* g, bool nanInput) {
  for (int k = 0; k < 6; ++k) {
    if (w[k] == g[k]) continue;
    if (nanInput && std::isnan(from_bits(w[k])) && std::isnan(from_bits(g[k]))) continue;
    return false;
  }
  return true;
}

void check_frame(f3 n) {
  f3 xa, ya, xb, yb;
  frame_branches(n, xa, ya);
  mi::diffuse_frame(n, xb, yb);
  const uint32_t w[6] = {bits(xa.x), bits(xa.y), bits(xa.z), bits(ya.x), bits(ya.y), bits(ya.z)};
  const uint32_t g[6] = {bits(xb.x), bits(xb.y), bits(xb.z), bits(yb.x), bits(yb.y), bits(yb.z)};
  if (!same_bits(w, g, std::isnan(n.x) || std::isnan(n.y) || std::isnan(n.z)) && failures++ < 10)
    std::printf("diffuse_frame differs for n = %08x %08x %08x: want %08x %08x %08x | %08x %08x %08x, got %08x %08x %08x | %08x %08x %08x\n", bits(n.x), bits(n.y), bits(n.z),
                w[0], w[1], w[2], w[3], w[4], w[5], g[0], g[1], g[2], g[3], g[4], g[5]);
}

void check_disc(float u1, float u2, const float* sinTbl) {
  float wx, wy, gx, gy;
  disc_reference(u1, u2, sinTbl, wx, wy);
  mi::sample_disc_concentric(u1, u2, sinTbl, gx, gy);
  if ((bits(wx) != bits(gx) || bits(wy) != bits(gy)) && failures++ < 10)
    std::printf("sample_disc_concentric differs for u = %08x %08x: want %08x %08x, got %08x %08x\n", bits(u1), bits(u2), bits(wx), bits(wy), bits(gx), bits(gy));
}

}  // namespace

int main() {
  // ---- the frame ----
  const float inf = INFINITY, qnan = from_bits(0x7FC00000u), nnan = from_bits(0xFFC00001u), pnan = from_bits(0x7FA00123u);
  const float special[] = {0.f, -0.f, from_bits(1u), -from_bits(1u), from_bits(0x007FFFFFu), -from_bits(0x007FFFFFu), from_bits(0x00800000u), 1e-30f, -1e-30f, 1e-19f, 0.5f, -0.5f,
                           0.70710678f, -0.70710678f, 1.f, -1.f, from_bits(0x3F7FFFFFu), from_bits(0x3F800001u), 3.f, -3.f, 1e19f, -1e19f, 3e38f, -3e38f, inf, -inf, qnan, nnan, pnan};
  long frames = 0;
  for (float x : special) for (float y : special) for (float z : special) { check_frame(mk(x, y, z)); ++frames; }
  // |n.x| == |n.y| ties (the compare is strict: a tie takes the second branch), either sign, and values one ulp to either side
  for (int k = 0; k < 200000; ++k) {
    const float v = (rnd() & 1u) ? rndUnit() : from_bits(rnd());
    const float z = rndUnit() * 2.f - 1.f;
    const float up = from_bits(bits(fabsf(v)) + 1u), dn = from_bits(bits(fabsf(v)) - 1u);
    for (float y : {v, -v, up, -up, dn, -dn}) { check_frame(mk(v, y, z)); check_frame(mk(y, v, z)); frames += 2; }
  }
  // random unit vectors (what a normal is), and random bit patterns
  for (int k = 0; k < 4000000; ++k) {
    const f3 v = mk(rndUnit() * 2.f - 1.f, rndUnit() * 2.f - 1.f, rndUnit() * 2.f - 1.f);
    check_frame(mi::normalized(v));
    ++frames;
  }
  for (int k = 0; k < 1000000; ++k) { check_frame(mk(from_bits(rnd()), from_bits(rnd()), from_bits(rnd()))); ++frames; }

  // ---- the concentric map ----
  float sinTbl[92];
  { static const uint32_t tblBits[92] = {MI_SIN_TABLE_BITS}; std::memcpy(sinTbl, tblBits, sizeof sinTbl); }
  const float half = 0.5f;
  std::vector<float> us = {0.f, half, 1.f, from_bits(bits(half) - 1u), from_bits(bits(half) + 1u), from_bits(bits(half) - 2u), from_bits(bits(half) + 2u), 0.25f, 0.75f,
                           from_bits(1u), from_bits(0x00800000u), from_bits(0x3F7FFFFFu), 1e-10f, 0.1f, 0.9f};
  long discs = 0;
  for (float a : us) for (float b : us) { check_disc(a, b, sinTbl); ++discs; }
  for (int k = 0; k < 2000000; ++k) {
    const float a = rndUnit();
    // |ux| == |uy|: u2 = u1 and u2 = 1 - u1 (exact for these 24-bit values), and the neighbours of both
    const float m = 1.f - a;
    for (float b : {a, m, from_bits(bits(a) + 1u), from_bits(bits(m) + 1u), a > 0.f ? from_bits(bits(a) - 1u) : a, m > 0.f ? from_bits(bits(m) - 1u) : m, rndUnit(), half}) {
      check_disc(a, b, sinTbl); check_disc(b, a, sinTbl);
      discs += 2;
    }
  }
  if (failures) { std::printf("diffuse_frame_check FAILED: %ld differences\n", failures); return 1; }
  std::printf("diffuse_frame_check OK: %ld frames, %ld disc samples, all bits equal\n", frames, discs);
  return 0;
}
