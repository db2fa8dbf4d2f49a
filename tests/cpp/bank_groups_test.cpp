// tests/cpp/bank_groups_test.cpp — ml::gpu::VoiceBank::processGroups (include/mlgpu/mldsp_gpu.hpp) against the two steps it
// replaces: operator() on an input expanded to one row per voice, then mlgpu_mixdown_groups. Built and run by
// tests/test_gpu_bank_groups.py; exits non-zero on the first failed REQUIRE.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "mlgpu/mldsp_gpu.hpp"

using namespace ml::gpu;

static int failures = 0;
#define REQUIRE(cond)                                             \
  do                                                              \
  {                                                               \
    if (!(cond))                                                  \
    {                                                             \
      printf("REQUIRE failed at line %d: %s\n", __LINE__, #cond); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

template <class F>
static bool throwsStatus(int status, F f)
{
  try
  {
    f();
  }
  catch (const Error& e)
  {
    return e.status == status;
  }
  return false;
}

int main()
{
  Engine engine(0);
  // 13 instruments of 16 resonators (208 voices: three full wavefronts and a quarter), one excitation row per instrument
  const size_t P = 16, N = 13, V = N * P, T = 2, S = T * kFloatsPerDSPVector;
  auto tune = [&](VoiceBank<Bandpass>& bank) {
    bank.clear();
    for (size_t v = 0; v < V; ++v) bank.coeffs<0>(v, Bandpass::makeCoeffs(0.01f + 0.02f * (float)(v % P), 0.05f + 0.001f * (float)(v / P)));
  };
  std::vector<float> excitation(N * S), expanded(V * S);  // [vector][row][64]
  uint32_t seed = 12345;
  for (float& x : excitation)
  {
    seed = seed * 0x0019660Du + 0x3C6EF35Fu;
    x = (float)(seed >> 8) * (2.f / 16777216.f) - 1.f;
  }
  for (size_t t = 0; t < T; ++t)
    for (size_t v = 0; v < V; ++v)
      memcpy(&expanded[(t * V + v) * 64], &excitation[(t * N + v / P) * 64], 64 * sizeof(float));

  VoiceBank<Bandpass> one(engine, V), two(engine, V);
  REQUIRE(one.fused());
  tune(one);
  tune(two);
  DeviceSignal in(engine, N, T), mix(engine, N, T, MLGPU_LAYOUT_ROWS);
  in.fromRows(excitation);
  one.processGroups(&in, (int)P, nullptr, (int)P, mix);

  DeviceSignal inV(engine, V, T), voices(engine, V, T), mix2(engine, N, T, MLGPU_LAYOUT_ROWS);
  inV.fromRows(expanded);
  two(inV, voices);
  engine.check(mlgpu_mixdown_groups(engine.handle(), voices.data(), voices.layout(), N, P, T, mix2.data(), mix2.layout()));
  const std::vector<float> a = mix.toRows(), b = mix2.toRows();
  REQUIRE(a.size() == N * S && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
  float peak = 0.f;
  for (float x : a) peak = fmaxf(peak, fabsf(x));
  REQUIRE(peak > 1e-4f && std::isfinite(peak));
  for (int i = 0; i < 2; ++i) REQUIRE(one.state(0, i) == two.state(0, i));

  // shapes: the input has voices / inGroup rows, the output voices / outGroup channels
  DeviceSignal wrong(engine, N + 1, T);
  REQUIRE(throwsStatus(MLGPU_ERR_INVALID, [&] { one.processGroups(&wrong, (int)P, nullptr, (int)P, mix); }));
  REQUIRE(throwsStatus(MLGPU_ERR_INVALID, [&] { one.processGroups(&in, (int)P, nullptr, (int)P, wrong); }));
  REQUIRE(throwsStatus(MLGPU_ERR_INVALID, [&] { one.processGroups(&in, (int)P, nullptr, 8, mix); }));
  REQUIRE(throwsStatus(MLGPU_ERR_INVALID, [&] { one.processGroups(nullptr, (int)P, nullptr, (int)P, mix); }));  // an input group without an input

  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
