// vad.hip — the spectral speech detector on the GPU (include/ohw.h, ohw_state_vad_frames): one speech probability per 10 ms
// frame of a recording.  This project's own rule, not Silero.  Three launches with plain kernel boundaries:
//   vad_band_kernel   e[t]: the 320 .. 3400 Hz band energy (bins 8..85 of the mel front end's 400-point DFT) in dB
//   vad_floor_kernel  a histogram of e (integer counts: LDS atomics per workgroup, then global ones; no order dependence)
//   vad_prob_kernel   head: the noise floor from the histogram's quantile; body: a 5-frame mean and a logistic
// Tiny next to a window's encode: a recording is n / 160 frames of 78 bins x 400 taps.
#include <algorithm>
#include <cmath>

#include "kernels.hpp"

namespace ohw {

constexpr int VAD_FR = 8;            // frames per workgroup, as mel_power_kernel
constexpr int VAD_THREADS = 128;
constexpr int VAD_K0 = 8, VAD_K1 = 85, VAD_NK = VAD_K1 - VAD_K0 + 1;     // 78 bins
constexpr int VAD_HIST_THREADS = 256;
constexpr int VAD_HIST_MAX_WG = 256;

__global__ __launch_bounds__(VAD_THREADS) void vad_band_kernel(VadParams p) {
  __shared__ float fr[N_FFT][VAD_FR];      // windowed frames, frame index fastest (broadcast reads)
  __shared__ float tw[2][N_FFT];
  __shared__ float pw[VAD_FR][VAD_NK + 2];
  const int64_t t0 = (int64_t)blockIdx.x * VAD_FR;
  const int tid = threadIdx.x;
  for (int i = tid; i < N_FFT; i += VAD_THREADS) { tw[0][i] = p.twiddle[i]; tw[1][i] = p.twiddle[N_FFT + i]; }
  for (int i = tid; i < N_FFT * VAD_FR; i += VAD_THREADS) {
    const int f = i / N_FFT, j = i % N_FFT;
    const int64_t t = t0 + f;
    int64_t pos = t * HOP - N_FFT / 2 + j;
    if (pos < 0) pos = -pos;                                   // reflected only at the recording's start
    float v = 0.0f;
    if (t < p.n_frames && pos < p.n) v = p.pcm[pos];           // zero from n on
    fr[j][f] = v * p.window[j];
  }
  __syncthreads();
  if (tid < VAD_NK) {
    const int k = VAD_K0 + tid;
    float re[VAD_FR], im[VAD_FR];
#pragma unroll
    for (int f = 0; f < VAD_FR; ++f) { re[f] = 0.f; im[f] = 0.f; }
    int idx = 0;
    for (int j = 0; j < N_FFT; ++j) {
      const float c = tw[0][idx], s = tw[1][idx];
      const f32x4 x0 = *(const f32x4*)&fr[j][0];
      const f32x4 x1 = *(const f32x4*)&fr[j][4];
      re[0] += x0.x * c; im[0] -= x0.x * s; re[1] += x0.y * c; im[1] -= x0.y * s;
      re[2] += x0.z * c; im[2] -= x0.z * s; re[3] += x0.w * c; im[3] -= x0.w * s;
      re[4] += x1.x * c; im[4] -= x1.x * s; re[5] += x1.y * c; im[5] -= x1.y * s;
      re[6] += x1.z * c; im[6] -= x1.z * s; re[7] += x1.w * c; im[7] -= x1.w * s;
      idx += k; if (idx >= N_FFT) idx -= N_FFT;
    }
#pragma unroll
    for (int f = 0; f < VAD_FR; ++f) pw[f][tid] = re[f] * re[f] + im[f] * im[f];
  }
  __syncthreads();
  if (tid < VAD_FR && t0 + tid < p.n_frames) {
    float acc = 0.f;
    for (int k = 0; k < VAD_NK; ++k) acc += pw[tid][k];        // a fixed order: bin 8 first
    p.energy[t0 + tid] = 10.0f * log10f(fmaxf(acc, 1e-10f));
  }
}

__device__ __forceinline__ int vad_bin(float e) {
  // clamp((int)floorf((e + 100) * 2), 0, 319), clamped as a float first so that no value overflows the conversion
  return (int)fminf(fmaxf(floorf((e + 100.0f) * 2.0f), 0.0f), (float)(VAD_BINS - 1));
}

__global__ __launch_bounds__(VAD_HIST_THREADS) void vad_floor_kernel(VadParams p) {
  __shared__ int32_t h[VAD_BINS];
  const int tid = threadIdx.x;
  for (int i = tid; i < VAD_BINS; i += VAD_HIST_THREADS) h[i] = 0;
  __syncthreads();
  for (int64_t t = (int64_t)blockIdx.x * VAD_HIST_THREADS + tid; t < p.n_frames; t += (int64_t)gridDim.x * VAD_HIST_THREADS)
    atomicAdd(&h[vad_bin(p.energy[t])], 1);
  __syncthreads();
  for (int i = tid; i < VAD_BINS; i += VAD_HIST_THREADS)
    if (h[i] != 0) atomicAdd(&p.hist[i], h[i]);
}

__global__ __launch_bounds__(256) void vad_prob_kernel(VadParams p) {
  __shared__ int32_t cnt[VAD_BINS];
  __shared__ float floor_s;
  const int tid = threadIdx.x;
  // head: the floor = the lower edge of the first bin whose cumulative count reaches the target.  Every workgroup finds it for
  // itself from the finished histogram (320 integers); workgroup 0 also stores it
  for (int i = tid; i < VAD_BINS; i += 256) cnt[i] = p.hist[i];
  __syncthreads();
  if (tid == 0) {
    int64_t cum = 0;
    int bin = VAD_BINS - 1;
    for (int i = 0; i < VAD_BINS; ++i) {
      cum += cnt[i];
      if (cum >= p.target) { bin = i; break; }
    }
    floor_s = -100.0f + 0.5f * (float)bin;
    if (blockIdx.x == 0) p.floor_db[0] = floor_s;
  }
  __syncthreads();
  const float fl = floor_s;
  const int64_t t = (int64_t)blockIdx.x * 256 + tid;
  if (t >= p.n_frames) return;
  const int64_t a = t - 2 < 0 ? 0 : t - 2, b = t + 2 >= p.n_frames ? p.n_frames - 1 : t + 2;
  float sum = 0.f;
  for (int64_t u = a; u <= b; ++u) sum += p.energy[u];         // ascending order
  const float es = sum / (float)(b - a + 1);
  p.prob[t] = 1.0f / (1.0f + expf(-(es - fl - p.margin_db) / p.slope_db));
}

void launch_vad_band(const VadParams& p, hipStream_t s) {
  const int64_t wgs = (p.n_frames + VAD_FR - 1) / VAD_FR;
  if (wgs < 1 || wgs > 0x7fffffff) throw Error(OHW_E_INVALID_ARG, "vad: bad frame count");
  hipLaunchKernelGGL(vad_band_kernel, dim3((unsigned)wgs), dim3(VAD_THREADS), 0, s, p);
  HIP_CHECK(hipGetLastError());
}

void launch_vad_floor_prob(const VadParams& p, hipStream_t s) {
  if (p.n_frames < 1 || p.target < 1 || p.target > p.n_frames) throw Error(OHW_E_INVALID_ARG, "vad: bad frame count or quantile target");
  HIP_CHECK(hipMemsetAsync(p.hist, 0, VAD_BINS * sizeof(int32_t), s));
  const int64_t hw = std::min<int64_t>((p.n_frames + VAD_HIST_THREADS - 1) / VAD_HIST_THREADS, VAD_HIST_MAX_WG);
  hipLaunchKernelGGL(vad_floor_kernel, dim3((unsigned)hw), dim3(VAD_HIST_THREADS), 0, s, p);
  hipLaunchKernelGGL(vad_prob_kernel, dim3((unsigned)((p.n_frames + 255) / 256)), dim3(256), 0, s, p);
  HIP_CHECK(hipGetLastError());
}

void vad_detector_check(const ohw_vad_detector& d) {
  if (!std::isfinite(d.floor_quantile) || !std::isfinite(d.margin_db) || !std::isfinite(d.slope_db) || !(d.floor_quantile > 0.0f) ||
      !(d.floor_quantile <= 1.0f) || !(d.slope_db > 0.0f))
    throw Error(OHW_E_INVALID_ARG, "vad detector: floor_quantile must be in (0, 1], slope_db above 0, and all three finite");
}

int32_t vad_floor_target(float q, int64_t n_frames) {
  const float c = ceilf(q * (float)n_frames);
  int64_t t = (int64_t)c;
  if (t < 1) t = 1;
  if (t > n_frames) t = n_frames;
  return (int32_t)t;
}

}  // namespace ohw
