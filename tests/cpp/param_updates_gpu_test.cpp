// tests/cpp/param_updates_gpu_test.cpp — ml::gpu::VoiceBank::applyUpdates (include/mlgpu/mldsp_gpu.hpp) against the staged
// whole-row route it stands beside: coeffs<I>(voice, c) for every voice of an instrument + commit(). Built and run by
// tests/test_gpu_param_updates.py; exits non-zero on the first failed REQUIRE.
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

static mlgpu_update coeffRecord(int proc, int idx, size_t first, size_t count, float value)
{
  mlgpu_update u{};
  u.node = proc;
  u.target = MLGPU_UPDATE_COEFF;
  u.index = (uint16_t)idx;
  u.first_voice = (uint32_t)first;
  u.n_voices = (uint32_t)count;
  memcpy(&u.bits, &value, 4);
  return u;
}

int main()
{
  Engine engine(0);
  // 13 instruments of 16 resonators (208 voices: three full wavefronts and a quarter)
  const size_t P = 16, N = 13, V = N * P, T = 2, S = T * kFloatsPerDSPVector;
  auto tune = [&](VoiceBank<Bandpass>& bank) {
    bank.clear();
    for (size_t v = 0; v < V; ++v) bank.coeffs<0>(v, Bandpass::makeCoeffs(0.01f + 0.02f * (float)(v % P), 0.05f + 0.001f * (float)(v / P)));
  };
  std::vector<float> noise(V * S);  // [vector][voice][64]
  uint32_t seed = 12345;
  for (float& x : noise)
  {
    seed = seed * 0x0019660Du + 0x3C6EF35Fu;
    x = (float)(seed >> 8) * (2.f / 16777216.f) - 1.f;
  }
  VoiceBank<Bandpass> one(engine, V), two(engine, V);
  tune(one);
  tune(two);
  two.reserveUpdates(64);
  DeviceSignal in(engine, V, T), outOne(engine, V, T), outTwo(engine, V, T);
  in.fromRows(noise);

  // three blocks; before the second and third a knob is turned on some instruments: the last one, one across the first wavefront's
  // end, and (third block) every voice
  for (int block = 0; block < 3; ++block)
  {
    std::vector<mlgpu_update> recs;
    auto turn = [&](size_t first, size_t count, float omega, float k) {
      const auto c = Bandpass::makeCoeffs(omega, k);
      for (size_t v = first; v < first + count; ++v) one.coeffs<0>(v, c);
      for (size_t i = 0; i < c.size(); ++i) recs.push_back(coeffRecord(0, (int)i, first, count, c[i]));
    };
    if (block == 1)
    {
      turn(V - P, P, 0.11f, 0.3f);
      turn(56, P, 0.07f, 0.2f);
    }
    if (block == 2) turn(0, V, 0.05f, 0.4f);
    two.applyUpdates(recs);
    one(in, outOne);
    two(in, outTwo);
    const std::vector<float> a = outOne.toRows(), b = outTwo.toRows();
    REQUIRE(a.size() == V * S && memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
    float peak = 0.f;
    for (float x : a) peak = fmaxf(peak, fabsf(x));
    REQUIRE(peak > 1e-4f && std::isfinite(peak));
    for (int i = 0; i < 2; ++i) REQUIRE(one.state(0, i) == two.state(0, i));
  }
  // the host copies followed the records: a staged change of one voice afterwards uploads rows that hold the updates
  one.coeffs<0>(3, Bandpass::makeCoeffs(0.2f, 0.5f));
  two.coeffs<0>(3, Bandpass::makeCoeffs(0.2f, 0.5f));
  one(in, outOne);
  two(in, outTwo);
  {
    const std::vector<float> a = outOne.toRows(), b = outTwo.toRows();
    REQUIRE(memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
  }

  // refusals come through as Error with the C ABI's status, and change nothing
  REQUIRE(throwsStatus(MLGPU_ERR_RANGE, [&] { two.applyUpdates({coeffRecord(0, 7, 0, 1, 1.f)}); }));
  REQUIRE(throwsStatus(MLGPU_ERR_RANGE, [&] { two.applyUpdates({coeffRecord(0, 0, V - 1, 2, 1.f)}); }));
  REQUIRE(throwsStatus(MLGPU_ERR_RANGE, [&] { two.applyUpdates(std::vector<mlgpu_update>(65, coeffRecord(0, 0, 0, 1, 1.f))); }));  // reserved: 64
  one(in, outOne);
  two(in, outTwo);
  {
    const std::vector<float> a = outOne.toRows(), b = outTwo.toRows();
    REQUIRE(memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
  }

  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
