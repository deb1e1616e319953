// tri_verdict_check.cpp — stand-alone check (no GPU) of the triangle test in csrc/tri_math.hpp, the text the kernels compile, against the
// test suite's CPU oracle: its o_ray_shear + o_intersect_triangle, looked up at run time in the shared library named on the command line
// (the product shares no code with the checker and does not link it; the three records below restate its argument layouts):
//   form A  intersect_triangle<DF, PRE, false> - the full verdict, the error bound's minima as min_abs3: the returned t bit for bit (a
//           NaN for a NaN: see same() below) for every case, and the barycentrics bit for bit wherever the oracle writes them (it does so only past its three early returns;
//           barycentrics it wrote are never all +0: det != 0 there, so some |e_i| >= |det| / 3.0001 and e_i * (1 / det) is at least 0.3,
//           infinite or NaN - all +0 is what it leaves behind when it returned early);
//   form B  intersect_triangle<DF, PRE, true> - the verdicts that t carries left out (POS): for tMin in {0, -1, 1e-3} and tCur in
//           {+inf, 1e30, 1, 1e-3, 0, NaN} the acceptance `t > 0 && t < inf && t > tMin && t < tCur` equals the oracle's, and so does
//           prim_hit's spelling of it, `t > 0 && t > tMin && t < tCur`; where the hit is accepted, t and the barycentrics bit for bit.
// PRE: the vertices and the origin arrive rotated for the shear axis (GLeafRot); both ways for every case. DF: the oracle's
// o_set_double_fallback 0 / 1 against the template argument false / true (a process-wide switch of the oracle: one pass each).
// The shear itself (make_shear against o_ray_shear) is compared on the way.
// Inputs: random triangles with rays aimed at them and beside them; coordinates and directions snapped to a coarse grid, repeated and
// collinear vertices among them, so that edge functions and det are exactly zero; origins on the triangle's plane and behind it; every one
// of the 15 inputs in turn set to each of +-0, +-denormal, +-3e38, +-inf, NaN over many base cases, and random pairs of them.
// No case is skipped. The program fails on any difference, and when fewer than 1e6 cases are accepted hits (tMin 0, tCur +inf) or fewer
// than 1e5 have a NaN among the operands of one of the four minima.
// Exit status 0 and "tri_verdict_check OK" = no difference. Built and run by tests/test_tri_verdict.py with the library's exact flags:
// tri_verdict_check <the oracle's shared library> [divisor of the case counts].
#include "../tri_math.hpp"

#include <dlfcn.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace {

using mi::f3;
using mi::mk;

// the oracle's records and entry points (C ABI)
struct ovec3 { float x, y, z; };
struct oray { ovec3 origin; float tMin; ovec3 direction; float tMax; };
struct oshear { ovec3 o; ovec3 dir; uint32_t ix, iy, iz; float sx, sy, sz; };
void (*o_ray_shear)(const oray*, oshear*);
float (*o_intersect_triangle)(ovec3, ovec3, ovec3, const oshear*, float, float*);
void (*o_set_double_fallback)(int);

uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
// Bit for bit, except that a NaN equals a NaN: where two NaNs of different sign meet in a commutative operation (-d.x / d.z against a NaN
// vertex, say) the one that comes out is the compiler's operand order - the oracle is C built by gcc -O3, this text C++ built by g++ -O2 -,
// and the device returns its canonical NaN whatever went in. Every value that is not NaN is compared by its bits, zeros' signs included.
bool same(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

struct Rnd {
  uint64_t s;
  uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
  float unit() { return (float)(next() >> 8) * (1.f / 16777216.f); }      // [0, 1)
  float sym(float r) { return (unit() * 2.f - 1.f) * r; }
  float grid() { return (float)((int)(next() % 33u) - 16) * 0.25f; }      // multiples of 1/4 in [-4, 4]
};

struct Case { float v[15]; };      // o, d, p0, p1, p2
f3 at(const Case& c, int k) { return mk(c.v[3 * k], c.v[3 * k + 1], c.v[3 * k + 2]); }
void put(Case& c, int k, f3 p) { c.v[3 * k] = p.x; c.v[3 * k + 1] = p.y; c.v[3 * k + 2] = p.z; }

const float kSpecials[9] = {0.f, -0.f, 1e-41f, -1e-41f, 3e38f, -3e38f, INFINITY, -INFINITY, NAN};

struct Tally {
  long cases = 0, hits = 0, nanMin = 0, zeroEdge = 0, zeroDet = 0, posReturnsMore = 0, failures = 0;
  void operator+=(const Tally& o) { cases += o.cases; hits += o.hits; nanMin += o.nanMin; zeroEdge += o.zeroEdge; zeroDet += o.zeroDet; posReturnsMore += o.posReturnsMore; failures += o.failures; }
};
std::atomic<long> printed{0};

void report(const char* what, const Case& c, float want, const float* wb, float got, f3 gb) {
  if (printed++ < 10) {
    std::printf("%s:", what);
    for (int k = 0; k < 15; ++k) std::printf(" %08x", bits(c.v[k]));
    std::printf(" | want %08x (%08x %08x %08x), got %08x (%08x %08x %08x)\n", bits(want), bits(wb[0]), bits(wb[1]), bits(wb[2]), bits(got), bits(gb.x), bits(gb.y), bits(gb.z));
  }
}

// Classification only (which cases the run has met, never what is right): whether an operand of one of the four minima is NaN, an edge
// function or det exactly zero - the first lines of the test on the oracle's shear.
void classify(const Case& c, const oshear& tf, Tally& n) {
  const f3 o = at(c, 0);
  f3 q[3];
  for (int k = 0; k < 3; ++k) {
    const f3 p = at(c, 2 + k) - o;
    q[k] = mk(mi::comp(p, tf.ix), mi::comp(p, tf.iy), mi::comp(p, tf.iz));
    q[k].x += tf.sx * q[k].z; q[k].y += tf.sy * q[k].z;
  }
  const float e0 = q[1].x * q[2].y - q[1].y * q[2].x, e1 = q[2].x * q[0].y - q[2].y * q[0].x, e2 = q[0].x * q[1].y - q[0].y * q[1].x;
  bool nan = std::isnan(e0) || std::isnan(e1) || std::isnan(e2);
  for (int k = 0; k < 3; ++k) nan = nan || std::isnan(q[k].x) || std::isnan(q[k].y) || std::isnan(q[k].z * tf.sz);
  n.nanMin += nan ? 1 : 0;
  n.zeroEdge += (e0 == 0.f || e1 == 0.f || e2 == 0.f) ? 1 : 0;
  n.zeroDet += (e0 + e1 + e2 == 0.f) ? 1 : 0;
}

const float kTMin[3] = {0.f, -1.f, 1e-3f};
const float kTCur[6] = {INFINITY, 1e30f, 1.f, 1e-3f, 0.f, NAN};

template <bool DF>
void check(const Case& c, Tally& n) {
  ++n.cases;
  const f3 o = at(c, 0), d = at(c, 1), p0 = at(c, 2), p1 = at(c, 3), p2 = at(c, 4);
  oray r;
  r.origin = {o.x, o.y, o.z}; r.tMin = 0.f; r.direction = {d.x, d.y, d.z}; r.tMax = INFINITY;
  oshear tf;
  o_ray_shear(&r, &tf);
  float wb[3];
  const float want = o_intersect_triangle({p0.x, p0.y, p0.z}, {p1.x, p1.y, p1.z}, {p2.x, p2.y, p2.z}, &tf, INFINITY, wb);
  classify(c, tf, n);

  const mi::Shear sh = mi::make_shear(d);
  if (sh.kz != tf.iz || !same(sh.sx, tf.sx) || !same(sh.sy, tf.sy) || !same(sh.sz, tf.sz)) {
    ++n.failures;
    report("make_shear differs", c, tf.sx, wb, sh.sx, mk(sh.sy, sh.sz, (float)sh.kz));
    return;
  }
  const bool wrote = bits(wb[0]) != 0u || bits(wb[1]) != 0u || bits(wb[2]) != 0u;
  const bool hit = want > 0.f && want < INFINITY;
  n.hits += hit ? 1 : 0;
  const f3 r0 = mi::permute_kz(p0, sh.kz), r1 = mi::permute_kz(p1, sh.kz), r2 = mi::permute_kz(p2, sh.kz), ro = mi::permute_kz(o, sh.kz);
  for (int pre = 0; pre < 2; ++pre) {
    // ---- form A ----
    f3 gb = mk(0.f, 0.f, 0.f);
    float got = pre ? mi::intersect_triangle<DF, true, false>(r0, r1, r2, ro, sh, gb.x, gb.y, gb.z) : mi::intersect_triangle<DF, false, false>(p0, p1, p2, o, sh, gb.x, gb.y, gb.z);
    if (!same(got, want) || (wrote && (!same(gb.x, wb[0]) || !same(gb.y, wb[1]) || !same(gb.z, wb[2])))) {
      ++n.failures;
      report(pre ? "form A, pre-rotated, differs" : "form A differs", c, want, wb, got, gb);
    }
    // ---- form B ----
    gb = mk(0.f, 0.f, 0.f);
    got = pre ? mi::intersect_triangle<DF, true, true>(r0, r1, r2, ro, sh, gb.x, gb.y, gb.z) : mi::intersect_triangle<DF, false, true>(p0, p1, p2, o, sh, gb.x, gb.y, gb.z);
    n.posReturnsMore += same(got, want) ? 0 : 1;
    for (float tMin : kTMin) for (float tCur : kTCur) {
      const bool accWant = want > 0.f && want < INFINITY && want > tMin && want < tCur;
      const bool accGot = got > 0.f && got < INFINITY && got > tMin && got < tCur;
      const bool accPrim = (got > 0.f) & (got > tMin) & (got < tCur);      // prim_hit's spelling
      const bool closer = (got > 0.f) & (got < tCur);                       // K1w's LEAF turn (tMin = 0)
      bool bad = accGot != accWant || accPrim != accWant || (tMin == 0.f && closer != accWant);
      if (accWant && !bad) bad = bits(got) != bits(want) || bits(gb.x) != bits(wb[0]) || bits(gb.y) != bits(wb[1]) || bits(gb.z) != bits(wb[2]);
      if (bad) {
        ++n.failures;
        report(pre ? "form B, pre-rotated, differs" : "form B differs", c, want, wb, got, gb);
        break;
      }
    }
  }
}

// ---- the inputs -----------------------------------------------------------------------------------------------------------------------
Case random_case(Rnd& g, int kind) {
  Case c;
  f3 p0 = mk(g.sym(4.f), g.sym(4.f), g.sym(4.f)), p1 = mk(g.sym(4.f), g.sym(4.f), g.sym(4.f)), p2 = mk(g.sym(4.f), g.sym(4.f), g.sym(4.f));
  if (kind % 4 == 3) { const float s = (kind & 4) ? 1e-3f : 1e3f; p1 = p0 + (p1 - p0) * s; p2 = p0 + (p2 - p0) * s; }      // tiny and huge triangles
  const f3 o = mk(g.sym(6.f), g.sym(6.f), g.sym(6.f));
  float a = g.unit(), b = g.unit();
  if (a + b > 1.f) { a = 1.f - a; b = 1.f - b; }
  if (kind % 8 == 5) b = 0.f;                                   // aimed at an edge
  if (kind % 8 == 6) { a = (kind & 8) ? 1.f : 0.f; b = 0.f; }   // aimed at a vertex
  const f3 q = p0 + (p1 - p0) * a + (p2 - p0) * b;
  f3 d = (kind & 1) ? q - o : mk(g.sym(1.f), g.sym(1.f), g.sym(1.f));
  if (kind % 16 == 9) d = mi::normalized(d);
  if (kind % 16 == 11) d = -d;                                   // the triangle behind the origin
  put(c, 0, o); put(c, 1, d); put(c, 2, p0); put(c, 3, p1); put(c, 4, p2);
  return c;
}
Case grid_case(Rnd& g, int kind) {
  Case c;
  f3 p0 = mk(g.grid(), g.grid(), g.grid()), p1 = mk(g.grid(), g.grid(), g.grid()), p2 = mk(g.grid(), g.grid(), g.grid());
  if (kind % 8 == 1) p2 = p1;                                            // zero area: a repeated vertex
  if (kind % 8 == 2) p2 = p0 + (p1 - p0) * 2.f;                          // collinear
  if (kind % 8 == 3) p1 = p2 = p0;                                       // a point
  if (kind % 8 == 4) { p1.z = p0.z; p2.z = p0.z; }                       // axis-aligned planes
  if (kind % 8 == 5) { p1.x = p0.x; p2.x = p0.x; }
  const f3 o = mk(g.grid(), g.grid(), g.grid());
  f3 d;
  if (kind % 4 == 0) d = mk((float)((int)(g.next() % 5u) - 2), (float)((int)(g.next() % 5u) - 2), (float)((int)(g.next() % 5u) - 2));      // axis-parallel and zero directions among them
  else {
    const uint32_t w = g.next() % 3u;                                    // at a vertex, along an edge, at the centre of an edge: exact on the grid
    const f3 q = w == 0 ? p0 : w == 1 ? p1 : (p0 + p1) * 0.5f;
    d = q - o;
    if (kind % 16 == 7) d = -d;
  }
  put(c, 0, o); put(c, 1, d); put(c, 2, p0); put(c, 3, p1); put(c, 4, p2);
  return c;
}
Case plane_case(Rnd& g, int kind) {
  Case c = (kind & 1) ? grid_case(g, kind >> 1) : random_case(g, kind >> 1);
  const f3 p0 = at(c, 2), p1 = at(c, 3), p2 = at(c, 4);
  float a = (kind & 2) ? g.unit() : g.sym(2.f), b = (kind & 2) ? g.unit() * (1.f - a) : g.sym(2.f);
  if (kind & 1) { a = (float)(g.next() % 5u) * 0.25f; b = (float)(g.next() % 5u) * 0.25f; }
  const f3 q = p0 + (p1 - p0) * a + (p2 - p0) * b;      // on the triangle's plane, inside or outside the triangle
  f3 d = at(c, 1);
  f3 o = q;
  if (kind % 8 >= 4) o = q + d * ((kind & 8) ? 1e-6f : (kind & 16) ? 0.25f : 1e-3f);      // behind the plane's crossing: t <= 0 or inside the error bound
  if (kind % 32 == 6) d = (p1 - p0) * g.sym(1.f) + (p2 - p0) * g.sym(1.f);                // in the plane
  put(c, 0, o); put(c, 1, d);
  return c;
}

template <bool DF>
void slice(unsigned t, unsigned threads, long nRandom, long nGrid, long nPlane, long nBase, long nPairs, Tally& n) {
  Rnd g{0x9e3779b97f4a7c15ull ^ (0xD1B54A32D192ED03ull * (t + 1u))};
  for (long k = t; k < nRandom; k += threads) check<DF>(random_case(g, (int)(k / threads)), n);
  for (long k = t; k < nGrid; k += threads) check<DF>(grid_case(g, (int)(k / threads)), n);
  for (long k = t; k < nPlane; k += threads) check<DF>(plane_case(g, (int)(k / threads)), n);
  for (long k = t; k < nBase; k += threads) {      // every input in turn set to every special value
    const int kind = (int)(k / threads);
    const Case base = (kind % 3 == 0) ? grid_case(g, kind) : (kind % 3 == 1) ? random_case(g, kind | 1) : plane_case(g, kind);
    for (int i = 0; i < 15; ++i) for (float s : kSpecials) { Case c = base; c.v[i] = s; check<DF>(c, n); }
  }
  for (long k = t; k < nPairs; k += threads) {     // random pairs (and now and then triples) of them
    const int kind = (int)(k / threads);
    Case c = (kind & 1) ? grid_case(g, kind) : random_case(g, kind | 1);
    c.v[g.next() % 15u] = kSpecials[g.next() % 9u];
    c.v[g.next() % 15u] = kSpecials[g.next() % 9u];
    if (kind % 8 == 0) c.v[g.next() % 15u] = kSpecials[g.next() % 9u];
    check<DF>(c, n);
  }
}

template <bool DF>
Tally pass(unsigned threads, long scale) {
  o_set_double_fallback(DF ? 1 : 0);
  std::vector<Tally> part(threads);
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < threads; ++t)
    pool.emplace_back([t, threads, scale, &part]() { slice<DF>(t, threads, 26000000 / scale, 14000000 / scale, 10000000 / scale, 30000 / scale, 6000000 / scale, part[t]); });
  for (auto& th : pool) th.join();
  Tally n;
  for (const Tally& p : part) n += p;
  return n;
}

}  // namespace

// argv[1]: the oracle's shared library; argv[2] (optional): a divisor of the case counts, for a quick look; the floors are divided with them
int main(int argc, char** argv) {
  const long scale = argc > 2 ? std::atol(argv[2]) : 1;
  if (argc < 2 || scale < 1) { std::printf("usage: tri_verdict_check <oracle library> [divisor >= 1]\n"); return 2; }
  void* lib = dlopen(argv[1], RTLD_NOW);
  if (!lib) { std::printf("tri_verdict_check FAILED: %s\n", dlerror()); return 2; }
  o_ray_shear = reinterpret_cast<decltype(o_ray_shear)>(dlsym(lib, "o_ray_shear"));
  o_intersect_triangle = reinterpret_cast<decltype(o_intersect_triangle)>(dlsym(lib, "o_intersect_triangle"));
  o_set_double_fallback = reinterpret_cast<decltype(o_set_double_fallback)>(dlsym(lib, "o_set_double_fallback"));
  if (!o_ray_shear || !o_intersect_triangle || !o_set_double_fallback) { std::printf("tri_verdict_check FAILED: %s lacks an entry point\n", argv[1]); return 2; }
  unsigned threads = std::thread::hardware_concurrency();
  threads = threads < 1u ? 1u : threads > 16u ? 16u : threads;
  long failures = 0;
  for (int df = 0; df < 2; ++df) {
    const Tally n = df ? pass<true>(threads, scale) : pass<false>(threads, scale);
    std::printf("double_fallback %d: %ld cases (each plain and pre-rotated, forms A and B), %ld accepted hits, %ld with a NaN operand in a minimum, %ld with a zero edge function, "
                "%ld with det == 0, %ld returns of form B that differ from the oracle's (all rejected), %ld differences\n", df, n.cases, n.hits, n.nanMin, n.zeroEdge, n.zeroDet, n.posReturnsMore, n.failures);
    failures += n.failures;
    if (n.cases < 50000000 / scale) { std::printf("tri_verdict_check FAILED: fewer than 5e7 cases\n"); return 1; }
    if (n.hits < 1000000 / scale) { std::printf("tri_verdict_check FAILED: fewer than 1e6 accepted hits\n"); return 1; }
    if (n.nanMin < 100000 / scale) { std::printf("tri_verdict_check FAILED: fewer than 1e5 cases with a NaN operand in a minimum\n"); return 1; }
  }
  o_set_double_fallback(0);
  if (failures) { std::printf("tri_verdict_check FAILED: %ld differences\n", failures); return 1; }
  std::printf("tri_verdict_check OK\n");
  return 0;
}
