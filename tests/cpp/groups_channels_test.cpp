// tests/cpp/groups_channels_test.cpp — ml::gpu::VoiceBank::processGroupsChannels (include/mlgpu/mldsp_gpu.hpp): a stereo mix per
// instrument, each channel against processGroups of an identical bank with that channel's gains. Built and run by
// tests/test_gpu_groups_channels.py; exits non-zero on the first failed REQUIRE.
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

using Voice = VoiceBank<SawGen, Bandpass, Gain>;

int main()
{
  Engine engine(0);
  // 13 instruments of 16 voices (208 voices: three full wavefronts and a quarter), a constant-power pan per voice
  const size_t P = 16, N = 13, V = N * P, T = 2, S = T * kFloatsPerDSPVector, C = 2;
  auto tune = [&](Voice& bank) {
    bank.clear();
    for (size_t v = 0; v < V; ++v)
    {
      bank.input(v, 55.f * powf(2.f, 5.f * (float)v / (float)V) / 48000.f);
      bank.coeffs<1>(v, Bandpass::makeCoeffs(0.01f + 0.02f * (float)(v % P), 0.3f + 0.001f * (float)(v / P)));
      bank.coeffs<2>(v, std::array<float, 1>{0.25f});
    }
  };
  std::vector<float> gains(C * V);
  for (size_t v = 0; v < V; ++v)
  {
    const float pan = (float)((v * 37) % V) / (float)V;
    gains[v] = cosf(1.5707963f * pan);
    gains[V + v] = sinf(1.5707963f * pan);
  }
  void* p = nullptr;
  engine.check(mlgpu_alloc(engine.handle(), gains.size() * sizeof(float), &p));
  float* const dGains = static_cast<float*>(p);
  engine.check(mlgpu_upload(engine.handle(), dGains, gains.data(), gains.size() * sizeof(float)));

  Voice stereo(engine, V), left(engine, V), right(engine, V);
  REQUIRE(stereo.fused());
  tune(stereo);
  tune(left);
  tune(right);
  // VOICE_MAJOR: the two channels' signals one after the other are rows 0 .. N - 1 and N .. 2 N - 1 of one signal
  DeviceSignal both(engine, C * N, T, MLGPU_LAYOUT_VOICE_MAJOR), l(engine, N, T, MLGPU_LAYOUT_VOICE_MAJOR), r(engine, N, T, MLGPU_LAYOUT_VOICE_MAJOR);
  stereo.processGroupsChannels(nullptr, 1, (int)C, dGains, (int)P, both);
  left.processGroups(nullptr, 1, dGains, (int)P, l);
  right.processGroups(nullptr, 1, dGains + V, (int)P, r);
  std::vector<float> got(C * N * S), wantL(N * S), wantR(N * S);
  engine.check(mlgpu_download(engine.handle(), got.data(), both.data(), both.bytes()));
  engine.check(mlgpu_download(engine.handle(), wantL.data(), l.data(), l.bytes()));
  engine.check(mlgpu_download(engine.handle(), wantR.data(), r.data(), r.bytes()));
  REQUIRE(memcmp(got.data(), wantL.data(), N * S * sizeof(float)) == 0);
  REQUIRE(memcmp(got.data() + N * S, wantR.data(), N * S * sizeof(float)) == 0);
  REQUIRE(memcmp(wantL.data(), wantR.data(), N * S * sizeof(float)) != 0);
  float peak = 0.f;
  for (float x : got) peak = fmaxf(peak, fabsf(x));
  REQUIRE(peak > 1e-4f && std::isfinite(peak));
  // the voices advanced once
  for (int i = 0; i < 2; ++i) REQUIRE(stereo.state(1, i) == left.state(1, i));
  REQUIRE(stereo.state(0, 0) == right.state(0, 0));

  // one channel is processGroups itself
  tune(stereo);
  tune(left);
  DeviceSignal one(engine, N, T, MLGPU_LAYOUT_VOICE_MAJOR);
  stereo.processGroupsChannels(nullptr, 1, 1, dGains, (int)P, one);
  left.processGroups(nullptr, 1, dGains, (int)P, l);
  engine.check(mlgpu_download(engine.handle(), got.data(), one.data(), one.bytes()));
  engine.check(mlgpu_download(engine.handle(), wantL.data(), l.data(), l.bytes()));
  REQUIRE(memcmp(got.data(), wantL.data(), N * S * sizeof(float)) == 0);

  // shapes: `out` has channels * voices / outGroup rows; the library's own refusals come through as Error
  REQUIRE(throwsStatus(MLGPU_ERR_INVALID, [&] { stereo.processGroupsChannels(nullptr, 1, (int)C, dGains, (int)P, one); }));
  REQUIRE(throwsStatus(MLGPU_ERR_INVALID, [&] { stereo.processGroupsChannels(nullptr, 1, (int)C, dGains, 8, both); }));
  REQUIRE(throwsStatus(MLGPU_ERR_INVALID, [&] { stereo.processGroupsChannels(nullptr, 1, (int)C, nullptr, (int)P, both); }));  // null gains
  DeviceSignal three(engine, 3 * N, T, MLGPU_LAYOUT_VOICE_MAJOR);
  REQUIRE(throwsStatus(MLGPU_ERR_UNSUPPORTED, [&] { stereo.processGroupsChannels(nullptr, 1, 3, dGains, (int)P, three); }));

  mlgpu_free(engine.handle(), dGains);
  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
