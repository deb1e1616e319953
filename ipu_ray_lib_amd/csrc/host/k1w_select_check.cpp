// k1w_select_check — the selection of K1w's builds (csrc/k1w_builds.hpp select_k1w), on the CPU.
//   k1w_select_check            sweeps every value of every K1wChoice field: the function is total, what it returns for a library is in
//                               that library's set, every build of a set is returned for some choice, and the shipped library with the
//                               options its SceneOptions::set accepts selects shipped builds only. Prints "k1w_select_check OK".
//   k1w_select_check -          reads situations from standard input, one per line as `field=value ...` (fields left out keep the
//                               defaults of a plain render of the shipped library), and prints the name of the build each selects.
// tests/test_k1w_builds.py builds and runs both.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "../k1w_builds.hpp"

using namespace mi;

static bool in_library(bool variants, K1wId id) {
  if (id == K1wId::RefusedFast) return true;
  if (id == K1wId::PathPool) return variants;
  return variants ? with_k1w<true>(id, [](auto) {}) : with_k1w<false>(id, [](auto) {});
}

static K1wChoice defaults() {
  K1wChoice c{};
  c.hasNodes = c.mergeTurns = c.leanHit = c.leafRot = c.defaultWeights = c.poolFits = true;
  c.kernelChoice = 1; c.wavesPerSimd = 6;
  return c;
}

static int sweep() {
  int bad = 0;
  unsigned long long seen[2] = {0, 0}, choices = 0;
  for (unsigned bits = 0; bits < (1u << 16); ++bits)
    for (int kernel = 0; kernel <= 3; ++kernel)
      for (int waves = 4; waves <= 7; ++waves) {
        K1wChoice c{};
        unsigned b = bits;
        for (bool* f : {&c.variants, &c.stats, &c.slots, &c.hasNormals, &c.rotLeaves, &c.hasNodes, &c.hotOn, &c.doubleFallback, &c.fast, &c.specLeaf, &c.mergeTurns,
                        &c.leanHit, &c.leafRot, &c.defaultWeights, &c.poolFits}) { *f = b & 1u; b >>= 1; }
        if (b) continue;      // (fifteen flags)
        c.kernelChoice = kernel; c.wavesPerSimd = waves;
        const K1wId id = select_k1w(c);
        ++choices;
        if ((unsigned)id > (unsigned)K1wId::RefusedFast) { printf("not an id: %u\n", (unsigned)id); return 1; }
        seen[c.variants] |= 1ull << (unsigned)id;
        if (!in_library(c.variants, id) && ++bad < 10) printf("%s is selected in the %s library, which has no such build\n", k1w_name(id), c.variants ? "variants" : "shipped");
        // what the shipped library's SceneOptions::set lets through
        const bool accepted = kernel <= 1 && waves == 6 && c.mergeTurns && !c.specLeaf && c.defaultWeights && !(c.fast && (c.stats || c.doubleFallback));
        if (!c.variants && accepted && !in_library(false, id) && ++bad < 10) printf("%s: not a shipped build\n", k1w_name(id));
      }
  for (int v = 0; v < 2; ++v)
    for (unsigned i = 0; i <= (unsigned)K1wId::RefusedFast; ++i)
      if (in_library(v, (K1wId)i) && !(seen[v] >> i & 1ull) && ++bad < 10) printf("%s is in the %s library and no choice selects it\n", k1w_name((K1wId)i), v ? "variants" : "shipped");
  if (!bad) printf("k1w_select_check OK: %llu choices\n", choices);
  return bad ? 1 : 0;
}

static int answer_stdin() {
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    K1wChoice c = defaults();
    for (char* tok = strtok(line, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) {
      char* eq = strchr(tok, '=');
      if (!eq) { printf("bad token %s\n", tok); return 2; }
      *eq = '\0';
      const std::string k(tok); const int v = atoi(eq + 1);
      if (k == "variants") c.variants = v; else if (k == "stats") c.stats = v; else if (k == "slots") c.slots = v; else if (k == "hasNormals") c.hasNormals = v;
      else if (k == "rotLeaves") c.rotLeaves = v; else if (k == "hasNodes") c.hasNodes = v; else if (k == "hotOn") c.hotOn = v; else if (k == "doubleFallback") c.doubleFallback = v;
      else if (k == "fast") c.fast = v; else if (k == "specLeaf") c.specLeaf = v; else if (k == "mergeTurns") c.mergeTurns = v; else if (k == "leanHit") c.leanHit = v;
      else if (k == "leafRot") c.leafRot = v; else if (k == "defaultWeights") c.defaultWeights = v; else if (k == "poolFits") c.poolFits = v;
      else if (k == "kernelChoice") c.kernelChoice = v; else if (k == "wavesPerSimd") c.wavesPerSimd = v;
      else { printf("unknown field %s\n", tok); return 2; }
    }
    printf("%s\n", k1w_name(select_k1w(c)));
  }
  return 0;
}

int main(int argc, char** argv) { return (argc > 1 && !strcmp(argv[1], "-")) ? answer_stdin() : sweep(); }
