// align.hip — word timestamps: cross-attention alignment (the published openai-whisper find_alignment) on the device.
//
// Three small kernels on data a state already holds after a decode (include/ohw.h, ohw_state_align):
//   tap      one workgroup per (window, listed head): the 8 query rows of a replay chunk against the head's resident cross K,
//            fp32 soft-max over the window's first n_keys keys, probabilities p[a][i][t] in fp32;
//   reduce   per (head, key column) the mean and the population standard deviation over the token rows, then per (token
//            row, key) the width-7 median along the keys of z = (p - mean) / std by selection, and the mean over the heads;
//   dtw      one workgroup per window, thread i owns token row i, anti-diagonal sweep with the last two diagonals in LDS,
//            trace codes as bytes in global scratch, one thread walks back and writes every row's first key.
// The reduction and the DTW have host twins (ohw_align_reduce_host, ohw_dtw_host) built from the SAME inline functions
// below, with floating-point contraction off: every value is a fixed sequence of IEEE fp32 operations, so the device and the
// host agree to the bit and the DTW's result does not depend on the order the cells are visited in.
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "model.hpp"

namespace ohw {
extern thread_local std::string g_last_error;                    // engine.hip

namespace {
template <typename F>
int al_guard(F&& f) {
  ApiScope api;
  try {
    f();
    return OHW_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "host allocation failed";
    return OHW_E_OOM;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return OHW_E_TRANSCRIBE;
  }
}
}  // namespace

// ---- the arithmetic, shared by the kernels and the host twins ---------------------------------------------------------------
// index j of a length-n axis padded as numpy.pad(mode="reflect") pads it (repeated reflection when the pad exceeds n - 1)
__host__ __device__ inline int al_reflect(int j, int n) {
  if (n <= 1) return 0;
  const int period = 2 * (n - 1);
  j %= period;
  if (j < 0) j += period;
  return j < n ? j : period - j;
}
// mean and population standard deviation of n values col[0], col[stride], ..: sequential fp32 sums, no fused multiply-add
__host__ __device__ inline void al_col_stats(const float* col, int64_t stride, int n, float* mean, float* sd) {
#pragma clang fp contract(off)
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += col[(int64_t)i * stride];
  const float mu = s / (float)n;
  float v = 0.f;
  for (int i = 0; i < n; ++i) {
    const float dlt = col[(int64_t)i * stride] - mu;
    v += dlt * dlt;
  }
  *mean = mu;
  *sd = sqrtf(v / (float)n);
}
__host__ __device__ inline float al_z(float p, float mean, float sd) {
  return sd == 0.f ? 0.f : (p - mean) / sd;
}
// the 4th smallest of 7 values: an insertion sort, comparisons only
__host__ __device__ inline float al_median7(float* v) {
  for (int i = 1; i < 7; ++i) {
    const float x = v[i];
    int j = i - 1;
    while (j >= 0 && v[j] > x) { v[j + 1] = v[j]; --j; }
    v[j + 1] = x;
  }
  return v[3];
}
// m of one (token row, key): prow = the row's probabilities of head 0, p_head floats between heads; stats [n_heads][ld_stat][2]
__host__ __device__ inline float al_m_value(const float* prow, int64_t p_head, const float* stats, int64_t ld_stat, int n_heads, int n_keys, int t) {
#pragma clang fp contract(off)
  float acc = 0.f;
  for (int a = 0; a < n_heads; ++a) {
    float v[7];
    for (int o = 0; o < 7; ++o) {
      const int tt = al_reflect(t + o - 3, n_keys);
      const float* stt = stats + ((int64_t)a * ld_stat + tt) * 2;
      v[o] = al_z(prow[(int64_t)a * p_head + tt], stt[0], stt[1]);
    }
    acc += al_median7(v);
  }
  return acc / (float)n_heads;
}
// one DTW cell (include/ohw.h): the strict-minimum rule, ties to the last candidate
__host__ __device__ inline float al_dtw_cell(float x, float c0, float c1, float c2, uint8_t* code) {
  float c;
  if (c0 < c1 && c0 < c2) { c = c0; *code = 0; }
  else if (c1 < c0 && c1 < c2) { c = c1; *code = 1; }
  else { c = c2; *code = 2; }
  return x + c;
}
// walk back from (n, n_keys): start[k] = the key at which the path first enters row k; trace has n_keys + 1 codes per row
__host__ __device__ inline void al_backtrace(const uint8_t* trace, int n, int n_keys, int32_t* start) {
  int i = n, j = n_keys;
  while (i > 0 || j > 0) {
    if (i > 0 && j > 0) start[i - 1] = j - 1;
    const int code = i == 0 ? 2 : j == 0 ? 1 : trace[(int64_t)i * (n_keys + 1) + j];
    if (code == 0) { --i; --j; }
    else if (code == 1) --i;
    else --j;
  }
}

// ---- tap ---------------------------------------------------------------------------------------------------------------------
constexpr int AL_THREADS = 256;

template <typename T>
__global__ __launch_bounds__(AL_THREADS) void align_tap_kernel(AlignTapParams p, AlignTapList list) {
  extern __shared__ __align__(16) float al_lds[];   // qs [8][64], then the logits [8][lds_stride]
  float* qs = al_lds;
  float* lg = al_lds + 8 * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, h = list.head[blockIdx.x], a = list.slot[blockIdx.x];
  int nk = p.n_keys[b];
  nk = nk < 1 ? 1 : nk > p.t_len ? p.t_len : nk > p.lds_stride ? p.lds_stride : nk;
  const int n_all = p.n_all ? p.n_all[b] : p.row0 + p.rows;
  int rows = p.rows;
  if (rows > n_all - p.row0) rows = n_all - p.row0;
  if (rows > p.row_cap - p.row0) rows = p.row_cap - p.row0;
  if (rows <= 0) return;                          // the whole workgroup: nothing of this chunk belongs to the window
  const int d = p.n_head * 64;
  const T* q = (const T*)p.q + (int64_t)b * p.rows * d + h * 64;
  for (int e = tid; e < 8 * 64; e += AL_THREADS) {
    const int i = e >> 6, c = e & 63;
    // 0.125 = 1 / sqrt(64), the scale of the layer's cross-attention; a power of two, so q * 0.125 is exact
    const float v = i < rows ? (float)q[(int64_t)i * d + c] * 0.125f : 0.f;
    qs[e] = v;
    if (p.q_out && i < rows) p.q_out[(((int64_t)b * p.row_cap + p.row0 + i) * p.n_slots + a) * 64 + c] = v;
  }
  __syncthreads();
  const T* kb = (const T*)p.xk + (((int64_t)b * p.n_head + h) * p.t_len << 6);
  for (int t = tid; t < nk; t += AL_THREADS) {
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll
    for (int c8 = 0; c8 < 8; ++c8) {
      const vec8_t<T> kf = *(const vec8_t<T>*)(kb + ((int64_t)t << 6) + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float kv = (float)kf[e];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += qs[i * 64 + c8 * 8 + e] * kv;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) lg[i * p.lds_stride + t] = acc[i];
  }
  __syncthreads();
  for (int i = wave; i < rows; i += AL_THREADS / 64) {
    float* row = lg + i * p.lds_stride;
    float mx = -INFINITY;
    for (int t = lane; t < nk; t += 64) mx = fmaxf(mx, row[t]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int t = lane; t < nk; t += 64) {
      const float e = expf(row[t] - mx);
      row[t] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    float* out = p.p + (int64_t)b * p.p_win + (int64_t)a * p.p_head + (int64_t)(p.row0 + i) * p.p_row;
    for (int t = lane; t < nk; t += 64) out[t] = row[t] / sum;
    for (int t = nk + lane; t < p.p_fill; t += 64) out[t] = 0.f;      // keys past n_keys: exactly 0
  }
}

template <typename T>
void launch_align_tap(const AlignTapParams& p, const AlignTapList& list, int windows, hipStream_t s) {
  if (list.n < 1 || windows < 1) return;
  if (list.n > OHW_ALIGN_MAX_HEADS || p.rows < 1 || p.rows > 8 || p.lds_stride < 1 || p.lds_stride > p.t_len || p.lds_stride > p.p_row ||
      p.p_fill > p.p_row || p.row0 < 0)
    throw Error(OHW_E_INVALID_ARG, "align tap: bad launch parameters");
  const size_t lds = (size_t)(8 * 64 + 8 * (size_t)p.lds_stride) * 4;
  if (lds > 64 * 1024) throw Error(OHW_E_INVALID_ARG, "align tap: " + std::to_string(p.lds_stride) + " keys x 8 rows exceed 64 KiB of LDS");
  hipLaunchKernelGGL((align_tap_kernel<T>), dim3(list.n, windows), dim3(AL_THREADS), lds, s, p, list);
  HIP_CHECK(hipGetLastError());
}
template void launch_align_tap<bf16_t>(const AlignTapParams&, const AlignTapList&, int, hipStream_t);
template void launch_align_tap<f16_t>(const AlignTapParams&, const AlignTapList&, int, hipStream_t);

// ---- reduce ------------------------------------------------------------------------------------------------------------------
// grid (key blocks, heads, windows): thread = one key column of one head
__global__ __launch_bounds__(AL_THREADS) void align_stats_kernel(AlignReduceParams p) {
  const int b = blockIdx.z, a = blockIdx.y, t = blockIdx.x * AL_THREADS + threadIdx.x;
  const int n_all = p.n_all[b] < p.n_prompt + p.max_rows ? p.n_all[b] : p.n_prompt + p.max_rows;
  const int nk = p.n_keys[b] < p.max_keys ? p.n_keys[b] : p.max_keys;
  if (n_all < 1 || t >= nk) return;
  float mean, sd;
  al_col_stats(p.p + (int64_t)b * p.p_win + (int64_t)a * p.p_head + t, p.p_row, n_all, &mean, &sd);
  float* st = p.stats + (((int64_t)b * p.n_heads + a) * p.ld_stat + t) * 2;
  st[0] = mean;
  st[1] = sd;
}
// grid (key blocks, kept rows, windows): thread = one (token row, key) of m
__global__ __launch_bounds__(AL_THREADS) void align_median_kernel(AlignReduceParams p) {
  const int b = blockIdx.z, k = blockIdx.y, t = blockIdx.x * AL_THREADS + threadIdx.x;
  const int n_all = p.n_all[b] < p.n_prompt + p.max_rows ? p.n_all[b] : p.n_prompt + p.max_rows;
  const int nk = p.n_keys[b] < p.max_keys ? p.n_keys[b] : p.max_keys;
  if (n_all < 1 || k >= n_all - p.n_prompt || t >= nk) return;
  const float* prow = p.p + (int64_t)b * p.p_win + (int64_t)(p.n_prompt + k) * p.p_row;
  p.m[(int64_t)b * p.m_win + (int64_t)k * p.m_row + t] =
      al_m_value(prow, p.p_head, p.stats + (int64_t)b * p.n_heads * p.ld_stat * 2, p.ld_stat, p.n_heads, nk, t);
}

void launch_align_reduce(const AlignReduceParams& p, int windows, hipStream_t s) {
  if (windows < 1) return;
  const int max_rows = p.max_rows, max_keys = p.max_keys;
  if (p.n_heads < 1 || p.n_heads > OHW_ALIGN_MAX_HEADS || max_rows < 1 || max_keys < 1 || max_keys > p.ld_stat || max_keys > p.m_row || max_keys > p.p_row ||
      p.n_prompt < 0)
    throw Error(OHW_E_INVALID_ARG, "align reduce: bad launch parameters");
  const int kb = (max_keys + AL_THREADS - 1) / AL_THREADS;
  hipLaunchKernelGGL(align_stats_kernel, dim3(kb, p.n_heads, windows), dim3(AL_THREADS), 0, s, p);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(align_median_kernel, dim3(kb, max_rows, windows), dim3(AL_THREADS), 0, s, p);
  HIP_CHECK(hipGetLastError());
}

// ---- dtw ---------------------------------------------------------------------------------------------------------------------
// cell (i, j) lies on diagonal i + j; diag[q][i] holds cost[i][dg - i] of the diagonals dg with dg % 3 == q.  A cell reads
// (i - 1, j - 1) two diagonals back and (i - 1, j), (i, j - 1) one back: one barrier per diagonal orders everything.
__global__ __launch_bounds__(AL_THREADS) void align_dtw_kernel(AlignDtwParams p) {
  extern __shared__ __align__(16) float al_diag[];   // [3][max_rows + 1]
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = p.n_rows[b] < p.max_rows ? p.n_rows[b] : p.max_rows;
  if (n < 1) return;
  int nk = p.n_keys[b] < p.max_keys ? p.n_keys[b] : p.max_keys;
  if (nk < 1) nk = 1;
  const int ld = p.max_rows + 1;
  const float* m = p.m + (int64_t)b * p.m_win;
  uint8_t* trace = p.trace + (int64_t)b * p.trace_win;
  for (int dg = 0; dg <= n + nk; ++dg) {
    float* cur = al_diag + (dg % 3) * ld;
    const float* p1 = al_diag + ((dg + 2) % 3) * ld;
    const float* p2 = al_diag + ((dg + 1) % 3) * ld;
    const int lo = dg - nk > 0 ? dg - nk : 0, hi = dg < n ? dg : n;
    for (int i = lo + tid; i <= hi; i += AL_THREADS) {
      const int j = dg - i;
      if (i == 0 || j == 0) { cur[i] = dg == 0 ? 0.f : INFINITY; continue; }
      uint8_t code;
      cur[i] = al_dtw_cell(-m[(int64_t)(i - 1) * p.m_row + (j - 1)], p2[i - 1], p1[i - 1], p1[i], &code);
      trace[(int64_t)i * (nk + 1) + j] = code;
    }
    __syncthreads();
  }
  if (tid == 0) al_backtrace(trace, n, nk, p.idx + (int64_t)b * p.idx_win);
}

void launch_align_dtw(const AlignDtwParams& p, int windows, hipStream_t s) {
  if (windows < 1) return;
  if (p.max_rows < 1 || p.max_rows > 8192 || p.max_keys < 1 || p.max_keys > p.m_row || p.trace_win < (int64_t)(p.max_rows + 1) * (p.max_keys + 1) ||
      p.idx_win < p.max_rows)
    throw Error(OHW_E_INVALID_ARG, "align dtw: bad launch parameters");
  hipLaunchKernelGGL(align_dtw_kernel, dim3(windows), dim3(AL_THREADS), (size_t)3 * (p.max_rows + 1) * 4, s, p);
  HIP_CHECK(hipGetLastError());
}

// ---- host twins ----------------------------------------------------------------------------------------------------------------
void align_reduce_host(const float* p, int n_heads, int n_all, int n_prompt, int n_keys, float* m_out) {
  if (!p || !m_out) throw Error(OHW_E_INVALID_ARG, "align reduce: null argument");
  if (n_heads < 1 || n_heads > OHW_ALIGN_MAX_HEADS) throw Error(OHW_E_INVALID_ARG, "align reduce: n_heads " + std::to_string(n_heads) + " outside 1.." + std::to_string(OHW_ALIGN_MAX_HEADS));
  if (n_keys < 1 || n_prompt < 0 || n_all <= n_prompt) throw Error(OHW_E_INVALID_ARG, "align reduce: needs n_keys >= 1 and 0 <= n_prompt < n_all");
  std::vector<float> stats((size_t)n_heads * n_keys * 2);
  for (int a = 0; a < n_heads; ++a)
    for (int t = 0; t < n_keys; ++t)
      al_col_stats(p + (int64_t)a * n_all * n_keys + t, n_keys, n_all, &stats[((size_t)a * n_keys + t) * 2], &stats[((size_t)a * n_keys + t) * 2 + 1]);
  for (int k = 0; k < n_all - n_prompt; ++k)
    for (int t = 0; t < n_keys; ++t)
      m_out[(int64_t)k * n_keys + t] = al_m_value(p + (int64_t)(n_prompt + k) * n_keys, (int64_t)n_all * n_keys, stats.data(), n_keys, n_heads, n_keys, t);
}

void dtw_host(const float* m, int n, int n_keys, int32_t* start_idx_out) {
  if (!m || !start_idx_out) throw Error(OHW_E_INVALID_ARG, "dtw: null argument");
  if (n < 1 || n_keys < 1) throw Error(OHW_E_INVALID_ARG, "dtw: needs n >= 1 and n_keys >= 1");
  const int64_t ld = n_keys + 1;
  std::vector<float> cost((size_t)(n + 1) * ld, INFINITY);
  std::vector<uint8_t> trace((size_t)(n + 1) * ld, 0);
  cost[0] = 0.f;
  for (int i = 1; i <= n; ++i)
    for (int j = 1; j <= n_keys; ++j)
      cost[(size_t)(i * ld + j)] = al_dtw_cell(-m[(int64_t)(i - 1) * n_keys + (j - 1)], cost[(size_t)((i - 1) * ld + j - 1)], cost[(size_t)((i - 1) * ld + j)],
                                               cost[(size_t)(i * ld + j - 1)], &trace[(size_t)(i * ld + j)]);
  al_backtrace(trace.data(), n, n_keys, start_idx_out);
}

}  // namespace ohw

using namespace ohw;

extern "C" {

int ohw_align_reduce_host(const float* p, int n_heads, int n_all, int n_prompt, int n_keys, float* m_out) {
  return al_guard([&] { align_reduce_host(p, n_heads, n_all, n_prompt, n_keys, m_out); });
}

int ohw_dtw_host(const float* m, int n, int n_keys, int32_t* start_idx_out) {
  return al_guard([&] { dtw_host(m, n, n_keys, start_idx_out); });
}

int ohw_dbg_align_probs(int dtype, const void* q, const void* xk, int rows, int n_head, int t_len, int n_keys, const int32_t* heads_host, int n_heads,
                        float* p_out_host, void* stream) {
  return al_guard([&] {
    if (!q || !xk || !heads_host || !p_out_host) throw Error(OHW_E_INVALID_ARG, "dbg_align_probs: null argument");
    if (dtype != OHW_DTYPE_BF16 && dtype != OHW_DTYPE_F16) throw Error(OHW_E_INVALID_ARG, "dbg_align_probs: dtype must be OHW_DTYPE_BF16 or OHW_DTYPE_F16");
    if (rows < 1 || rows > 8 || n_head < 1 || t_len < 1 || n_keys < 1 || n_keys > t_len) throw Error(OHW_E_INVALID_ARG, "dbg_align_probs: needs 1 <= rows <= 8, 1 <= n_keys <= t_len");
    if (n_heads < 1 || n_heads > OHW_ALIGN_MAX_HEADS) throw Error(OHW_E_INVALID_ARG, "dbg_align_probs: n_heads outside 1.." + std::to_string(OHW_ALIGN_MAX_HEADS));
    AlignTapList list{};
    list.n = n_heads;
    for (int a = 0; a < n_heads; ++a) {
      if (heads_host[a] < 0 || heads_host[a] >= n_head) throw Error(OHW_E_INVALID_ARG, "dbg_align_probs: head " + std::to_string(a) + " is outside the model");
      list.slot[a] = (int16_t)a;
      list.head[a] = (int16_t)heads_host[a];
    }
    hipStream_t s = (hipStream_t)stream;
    DevBuf nk, pbuf;
    nk.alloc(4);
    const size_t n_out = (size_t)n_heads * rows * t_len;
    pbuf.alloc(n_out * 4);
    HIP_CHECK(hipMemcpyAsync(nk.p, &n_keys, 4, hipMemcpyHostToDevice, s));
    AlignTapParams p{};
    p.q = q; p.xk = xk; p.n_head = n_head; p.t_len = t_len; p.rows = rows; p.row0 = 0; p.row_cap = rows; p.lds_stride = n_keys;
    p.n_keys = nk.as<int32_t>(); p.n_all = nullptr;
    p.p = pbuf.as<float>(); p.p_win = 0; p.p_head = (int64_t)rows * t_len; p.p_row = t_len; p.p_fill = t_len;
    p.q_out = nullptr; p.n_slots = n_heads;
    if (dtype == OHW_DTYPE_BF16) launch_align_tap<bf16_t>(p, list, 1, s);
    else launch_align_tap<f16_t>(p, list, 1, s);
    HIP_CHECK(hipMemcpyAsync(p_out_host, pbuf.p, n_out * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int ohw_dbg_align_reduce(int device, const float* p_host, int n_heads, int n_all, int n_prompt, int n_keys, float* m_out_host) {
  return al_guard([&] {
    if (!p_host || !m_out_host) throw Error(OHW_E_INVALID_ARG, "dbg_align_reduce: null argument");
    if (n_heads < 1 || n_heads > OHW_ALIGN_MAX_HEADS) throw Error(OHW_E_INVALID_ARG, "dbg_align_reduce: n_heads outside 1.." + std::to_string(OHW_ALIGN_MAX_HEADS));
    if (n_keys < 1 || n_prompt < 0 || n_all <= n_prompt) throw Error(OHW_E_INVALID_ARG, "dbg_align_reduce: needs n_keys >= 1 and 0 <= n_prompt < n_all");
    HIP_CHECK(hipSetDevice(device));
    const int n = n_all - n_prompt;
    DevBuf pb, stats, mb, cnt;
    pb.alloc((size_t)n_heads * n_all * n_keys * 4);
    stats.alloc((size_t)n_heads * n_keys * 2 * 4);
    mb.alloc((size_t)n * n_keys * 4);
    cnt.alloc(8);
    const int32_t c[2] = {n_all, n_keys};
    HIP_CHECK(hipMemcpy(pb.p, p_host, pb.bytes, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(cnt.p, c, 8, hipMemcpyHostToDevice));
    AlignReduceParams p{};
    p.p = pb.as<float>(); p.p_win = 0; p.p_head = (int64_t)n_all * n_keys; p.p_row = n_keys;
    p.stats = stats.as<float>(); p.ld_stat = n_keys; p.n_heads = n_heads; p.n_prompt = n_prompt;
    p.n_all = cnt.as<int32_t>(); p.n_keys = cnt.as<int32_t>() + 1;
    p.m = mb.as<float>(); p.m_win = 0; p.m_row = n_keys; p.max_rows = n; p.max_keys = n_keys;
    launch_align_reduce(p, 1, nullptr);
    HIP_CHECK(hipMemcpy(m_out_host, mb.p, mb.bytes, hipMemcpyDeviceToHost));
  });
}

int ohw_dbg_dtw(int device, const float* m_host, int n, int n_keys, int32_t* start_idx_out) {
  return al_guard([&] {
    if (!m_host || !start_idx_out) throw Error(OHW_E_INVALID_ARG, "dbg_dtw: null argument");
    if (n < 1 || n > 8192 || n_keys < 1) throw Error(OHW_E_INVALID_ARG, "dbg_dtw: needs 1 <= n <= 8192 and n_keys >= 1");
    HIP_CHECK(hipSetDevice(device));
    DevBuf mb, trace, idx, cnt;
    mb.alloc((size_t)n * n_keys * 4);
    trace.alloc((size_t)(n + 1) * (n_keys + 1));
    idx.alloc((size_t)n * 4);
    cnt.alloc(8);
    const int32_t c[2] = {n, n_keys};
    HIP_CHECK(hipMemcpy(mb.p, m_host, mb.bytes, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(cnt.p, c, 8, hipMemcpyHostToDevice));
    AlignDtwParams p{};
    p.m = mb.as<float>(); p.m_win = 0; p.m_row = n_keys; p.n_rows = cnt.as<int32_t>(); p.n_keys = cnt.as<int32_t>() + 1;
    p.trace = trace.as<uint8_t>(); p.trace_win = (int64_t)trace.bytes; p.idx = idx.as<int32_t>(); p.idx_win = n; p.max_rows = n; p.max_keys = n_keys;
    launch_align_dtw(p, 1, nullptr);
    HIP_CHECK(hipMemcpy(start_idx_out, idx.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
