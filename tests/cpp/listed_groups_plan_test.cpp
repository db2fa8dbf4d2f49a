// The lane plan of the listed group sum (madronalib_amd/csrc/voice_list.cpp: mlvl::planGroups) without a device: built by g++ with the
// address and undefined-behaviour sanitizers from that one file by tests/test_voice_list_groups_cpu.py, and run directly.
//   listed_groups_plan_test LISTS   - LISTS is a text file, one list per line: "name K v0 v1 ... v[K-1]" (the tests' named lists)
// Every named list at G = 2, 4, 8, 16, the table of N / pads / J modelled for them, and 2 000 seeded random lists must satisfy:
//   the voices appear in list order, each once, with their list position; pads only between a segment's end and the next multiple
//   of 64; no segment crosses a multiple of 64; rows 0 .. J-1 in order, one per segment; rank and length consistent; M the distinct
//   list[i] / G; N <= 64 ceil(K / (65 - G)); the plan arrays written nowhere past N (and the groups array nowhere past J); every
//   voice of a bank of whole groups: no pads, N = V, J = V / G.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../madronalib_amd/csrc/voice_list.hpp"

static int failures = 0;
#define CHECK(cond, ...)                \
  do                                    \
  {                                     \
    if (!(cond))                        \
    {                                   \
      if (++failures <= 20)             \
      {                                 \
        printf("FAILED %s: ", #cond);   \
        printf(__VA_ARGS__);            \
        printf("\n");                   \
      }                                 \
      return;                           \
    }                                   \
  } while (0)

struct Result
{
  size_t N{0}, pads{0}, J{0};
};

static void checkPlan(const char* what, const std::vector<uint32_t>& list, unsigned G, Result* out = nullptr)
{
  const size_t K = list.size(), cap = mlvl::maxPlanLanes(K, G);
  CHECK(cap % 64 == 0 && cap == 64 * ((K + 64 - G) / (65 - G)), "%s G=%u: the reserve's size", what, G);
  const uint32_t canary = 0xA5A5A5A5u;
  // exactly the promised sizes: the sanitizer sees a write past them, the canaries a write inside them that the plan does not own
  std::vector<uint32_t> lanes(mlvl::kLaneWords * cap, canary), groups(K, canary);
  const mlvl::LanePlan plan = mlvl::planGroups(list.data(), K, G, lanes.data(), groups.data());
  const size_t N = plan.lanes, J = plan.groups;
  CHECK(N <= cap, "%s G=%u: N %zu > %zu", what, G, N, cap);
  CHECK(J <= K, "%s G=%u: J", what, G);
  for (size_t w = mlvl::kLaneWords * N; w < lanes.size(); ++w) CHECK(lanes[w] == canary, "%s G=%u: a word past N written", what, G);
  for (size_t j = J; j < K; ++j) CHECK(groups[j] == canary, "%s G=%u: a group past J written", what, G);
  size_t i = 0, row = 0, pads = 0, l = 0;
  while (l < N)
  {
    const uint32_t* w = &lanes[mlvl::kLaneWords * l];
    if (w[0] == mlvl::kPad)
    {
      // a run of pads: from a segment's end to the next multiple of 64, and a segment that would not have fitted follows
      CHECK(l % 64 != 0, "%s G=%u: a pad at the start of a wavefront (lane %zu)", what, G, l);
      const size_t start = l;
      while (l < N && lanes[mlvl::kLaneWords * l] == mlvl::kPad)
      {
        CHECK(lanes[mlvl::kLaneWords * l + 1] == 0 && lanes[mlvl::kLaneWords * l + 2] == 0 && lanes[mlvl::kLaneWords * l + 3] == 0, "%s G=%u: pad words", what, G);
        ++l;
        ++pads;
      }
      CHECK(l < N && l % 64 == 0, "%s G=%u: pads from lane %zu end at lane %zu", what, G, start, l);
      CHECK(l - start < G, "%s G=%u: %zu pads", what, G, l - start);
      const unsigned nextLen = lanes[mlvl::kLaneWords * l + 3] >> 8;
      CHECK(nextLen > l - start, "%s G=%u: the segment after the pads (%u lanes) would have fitted into %zu", what, G, nextLen, l - start);
      continue;
    }
    // a segment
    const unsigned len = w[3] >> 8;
    CHECK(len >= 1 && len <= G, "%s G=%u: length %u at lane %zu", what, G, len, l);
    CHECK(l / 64 == (l + len - 1) / 64, "%s G=%u: the segment at lane %zu (%u lanes) crosses a wavefront", what, G, l, len);
    CHECK(l + len <= N && i + len <= K, "%s G=%u: the segment at lane %zu runs past the end", what, G, l);
    for (unsigned r = 0; r < len; ++r)
    {
      const uint32_t* s = &lanes[mlvl::kLaneWords * (l + r)];
      CHECK(s[0] == list[i + r] && s[1] == i + r, "%s G=%u: lane %zu is not list position %zu", what, G, l + r, i + r);
      CHECK(s[2] == row, "%s G=%u: lane %zu row %u, want %zu", what, G, l + r, s[2], row);
      CHECK((s[3] & 0xFF) == r && (s[3] >> 8) == len, "%s G=%u: lane %zu rank / length", what, G, l + r);
      CHECK(s[0] / G == list[i] / G, "%s G=%u: lane %zu is another instrument's voice", what, G, l + r);
    }
    // maximal: the neighbours belong to other instruments
    CHECK(i == 0 || list[i - 1] / G != list[i] / G, "%s G=%u: the segment at lane %zu continues the one before", what, G, l);
    CHECK(i + len == K || list[i + len] / G != list[i] / G, "%s G=%u: the segment at lane %zu stops early", what, G, l);
    CHECK(row < J && groups[row] == list[i] / G, "%s G=%u: M[%zu]", what, G, row);
    i += len;
    l += len;
    ++row;
  }
  CHECK(i == K && row == J && l == N, "%s G=%u: %zu of %zu voices, %zu of %zu rows", what, G, i, K, row, J);
  CHECK(N == K + pads, "%s G=%u: N", what, G);
  CHECK(K == 0 || lanes[mlvl::kLaneWords * (N - 1)] != mlvl::kPad, "%s G=%u: N ends on a pad", what, G);
  if (out) *out = Result{N, pads, J};
}

static void expectTable(const char* name, unsigned G, const Result& got, size_t N, size_t pads, size_t J)
{
  if (got.N != N || got.pads != pads || got.J != J)
  {
    ++failures;
    printf("FAILED table %s G=%u: N %zu pads %zu J %zu, want %zu %zu %zu\n", name, G, got.N, got.pads, got.J, N, pads, J);
  }
}

int main(int argc, char** argv)
{
  if (argc < 2)
  {
    printf("usage: listed_groups_plan_test LISTS\n");
    return 2;
  }
  const unsigned sizes[4] = {2, 4, 8, 16};
  std::ifstream in(argv[1]);
  std::string line;
  int named = 0, tabled = 0;
  while (std::getline(in, line))
  {
    std::istringstream ss(line);
    std::string name;
    size_t K = 0;
    if (!(ss >> name >> K)) continue;
    std::vector<uint32_t> list(K);
    for (size_t i = 0; i < K; ++i) ss >> list[i];
    if (!ss)
    {
      ++failures;
      printf("FAILED reading list %s\n", name.c_str());
      continue;
    }
    ++named;
    for (unsigned G : sizes)
    {
      Result r;
      checkPlan(name.c_str(), list, G, &r);
      struct Row
      {
        const char* name;
        unsigned G;
        size_t N, pads, J;
      };
      static const Row table[] = {{"k2100", 2, 2120, 20, 1167}, {"k2100", 4, 2140, 40, 587}, {"k2100", 8, 2212, 112, 294}, {"k2100", 16, 2348, 248, 147},
                                  {"straddle", 16, 76, 2, 71},  {"fit", 16, 81, 0, 63},      {"all", 16, 2352, 0, 147}};
      for (const Row& t : table)
        if (name == t.name && G == t.G)
        {
          expectTable(t.name, G, r, t.N, t.pads, t.J);
          ++tabled;
        }
      if (name == "all") expectTable("all", G, r, K, 0, K / G);
      if (name == "empty") expectTable("empty", G, r, 0, 0, 0);
    }
  }
  if (named < 7 || tabled != 7)
  {
    ++failures;
    printf("FAILED: %d named lists, %d table rows checked (want at least 7, and 7)\n", named, tabled);
  }

  // every voice of banks of whole groups: no pads
  for (unsigned G : sizes)
    for (size_t V : {(size_t)G, (size_t)64, (size_t)80, (size_t)4096})
    {
      std::vector<uint32_t> all(V);
      for (size_t v = 0; v < V; ++v) all[v] = (uint32_t)v;
      Result r;
      checkPlan("every voice", all, G, &r);
      expectTable("every voice", G, r, V, 0, V / G);
    }

  // 2 000 seeded random lists: densities from a few voices to nearly all, banks from one group to a few thousand voices
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&rng]() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return rng;
  };
  for (int c = 0; c < 2000; ++c)
  {
    const unsigned G = sizes[next() % 4];
    const size_t V = G * (1 + next() % 300);
    const unsigned density = 1 + (unsigned)(next() % 100);  // percent
    std::vector<uint32_t> list;
    for (size_t v = 0; v < V; ++v)
      if (next() % 100 < density) list.push_back((uint32_t)v);
    char what[64];
    snprintf(what, sizeof(what), "random %d (V %zu, %u %%)", c, V, density);
    checkPlan(what, list, G);
  }
  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
