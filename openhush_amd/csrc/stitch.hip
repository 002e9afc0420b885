// stitch.hip — stitched windows: the merge rule between overlapped fixed cuts, as a device kernel and its host twin
// (include/ohw.h states the rule; DESIGN.md sections 6 and 9).
//
//   stitch_kernel   one workgroup of 256 threads per seam.  The two windows' text tokens are staged in LDS; thread t takes the
//                   shifts t + 1, t + 257, ... in ascending order, counts the matches of each and keeps its own first best
//                   (score, shift, matches); the block reduction keeps the greater score and, on equal scores, the smaller
//                   shift - the sequential scan's first maximum.  Neighbouring threads hold neighbouring shifts, so at every
//                   position of the count they read neighbouring LDS words (left) or neighbouring words / one word (right).
// The score is a fixed sequence of IEEE float64 operations (two divisions, one addition, contraction off) on the device and
// on the host, so the two agree with numpy to the bit.  The plan, the ranges and the segment clip are host rules only.
#include <climits>
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
int st_guard(F&& f) {
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

constexpr int STITCH_THREADS = 256;
constexpr int STITCH_MAX_STRIDE = 4096;      // 2 * 4096 ids = 32 KiB of LDS
constexpr int STITCH_NONE = INT_MAX;         // the shift of "no candidate": loses every tie

// ---- the arithmetic, shared by the kernel and the host twin ----
struct SeamBest { double score; int shift, matches; };

__host__ __device__ inline double seam_score(int m, int i) {
#pragma clang fp contract(off)
  const double ratio = (double)m / (double)i;
  const double eps = (double)i / 10000.0;
  return ratio + eps;
}
// matches of shift i between left[0 .. L) and right[0 .. R)
__host__ __device__ inline int seam_matches(const int32_t* left, int L, const int32_t* right, int R, int i) {
  const int ls = L - i > 0 ? L - i : 0, le = L + R - i < L ? L + R - i : L, rs = i - L > 0 ? i - L : 0;
  int m = 0;
  for (int j = 0; j < le - ls; ++j) m += left[ls + j] == right[rs + j] ? 1 : 0;
  return m;
}
// a candidate of a later shift against the best so far of earlier ones
__host__ __device__ inline void seam_take(SeamBest& best, int m, int i) {
  if (m <= 1) return;
  const double s = seam_score(m, i);
  if (s > best.score) best = SeamBest{s, i, m};
}
// two partial results of disjoint shift sets: the greater score, on equal scores the smaller shift
__host__ __device__ inline SeamBest seam_merge(const SeamBest& a, const SeamBest& b) {
  return (b.score > a.score || (b.score == a.score && b.shift < a.shift)) ? b : a;
}
__host__ __device__ inline ohw_seam seam_record(int left_window, const SeamBest& best, int L, int R) {
  if (best.shift == STITCH_NONE) return ohw_seam{left_window, 0, 0, L, 0, L, R, 0};
  const int i = best.shift;
  const int ls = L - i > 0 ? L - i : 0, le = L + R - i < L ? L + R - i : L, rs = i - L > 0 ? i - L : 0, re = R < i ? R : i;
  return ohw_seam{left_window, i, best.matches, (ls + le) / 2, (rs + re) / 2, L, R, 0};
}

__global__ __launch_bounds__(STITCH_THREADS) void stitch_kernel(const int32_t* __restrict__ tok, int stride, const int32_t* __restrict__ n_text,
                                                                 int n_seams, ohw_seam* __restrict__ out) {
  extern __shared__ int32_t st_lds[];
  __shared__ double w_score[STITCH_THREADS / 64];
  __shared__ int w_shift[STITCH_THREADS / 64], w_matches[STITCH_THREADS / 64];
  const int s = (int)blockIdx.x, t = (int)threadIdx.x;
  if (s >= n_seams) return;
  const int nl = n_text[s], nr = n_text[s + 1];
  const int L = nl < 0 ? 0 : nl > stride ? stride : nl, R = nr < 0 ? 0 : nr > stride ? stride : nr;
  int32_t* left = st_lds;
  int32_t* right = st_lds + stride;
  // nothing behind n_text is read
  for (int j = t; j < L; j += STITCH_THREADS) left[j] = tok[(size_t)s * stride + j];
  for (int j = t; j < R; j += STITCH_THREADS) right[j] = tok[(size_t)(s + 1) * stride + j];
  __syncthreads();
  SeamBest best{0.0, STITCH_NONE, 0};
  for (int i = t + 1; i <= L + R - 1; i += STITCH_THREADS) seam_take(best, seam_matches(left, L, right, R, i), i);
  // within a wave by shuffles
  for (int d = 32; d >= 1; d >>= 1) {
    SeamBest o;
    o.score = __shfl_xor(best.score, d, 64);
    o.shift = __shfl_xor(best.shift, d, 64);
    o.matches = __shfl_xor(best.matches, d, 64);
    best = seam_merge(best, o);
  }
  // across the four waves through LDS
  if ((t & 63) == 0) { w_score[t >> 6] = best.score; w_shift[t >> 6] = best.shift; w_matches[t >> 6] = best.matches; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < STITCH_THREADS / 64; ++w) best = seam_merge(best, SeamBest{w_score[w], w_shift[w], w_matches[w]});
    out[s] = seam_record(s, best, L, R);
  }
}

void check_seam_args(const char* what, const int32_t* tok, int stride, const int32_t* n_text, int n_windows, const ohw_seam* out) {
  if (n_windows < 0 || stride < 1 || stride > STITCH_MAX_STRIDE)
    throw Error(OHW_E_INVALID_ARG, std::string(what) + ": needs n_windows >= 0 and 1 <= stride <= " + std::to_string(STITCH_MAX_STRIDE));
  if (n_windows > 0 && (!tok || !n_text)) throw Error(OHW_E_INVALID_ARG, std::string(what) + ": null argument");
  if (n_windows > 1 && !out) throw Error(OHW_E_INVALID_ARG, std::string(what) + ": null output");
  for (int w = 0; w < n_windows; ++w)
    if (n_text[w] < 0 || n_text[w] > stride)
      throw Error(OHW_E_INVALID_ARG, std::string(what) + ": window " + std::to_string(w) + " holds " + std::to_string(n_text[w]) + " text tokens, the stride is " + std::to_string(stride));
}

void stitch_device(int device, const int32_t* tok, int stride, const int32_t* n_text, int n_windows, int n_guard, int32_t sentinel, ohw_seam* out) {
  const int n_seams = n_windows - 1;
  HIP_CHECK(hipSetDevice(device));
  DevBuf tb, nb, ob;
  tb.alloc((size_t)n_windows * stride * 4);
  nb.alloc((size_t)n_windows * 4);
  ob.alloc((size_t)(n_seams + n_guard) * sizeof(ohw_seam));
  HIP_CHECK(hipMemcpy(tb.p, tok, (size_t)n_windows * stride * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(nb.p, n_text, (size_t)n_windows * 4, hipMemcpyHostToDevice));
  if (n_guard > 0) {
    std::vector<int32_t> fill((size_t)(n_seams + n_guard) * 8, sentinel);
    HIP_CHECK(hipMemcpy(ob.p, fill.data(), fill.size() * 4, hipMemcpyHostToDevice));
  }
  stitch_kernel<<<dim3((unsigned)n_seams), dim3(STITCH_THREADS), (size_t)2 * stride * 4, nullptr>>>(tb.as<int32_t>(), stride, nb.as<int32_t>(), n_seams,
                                                                                                   ob.as<ohw_seam>());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpy(out, ob.p, (size_t)(n_seams + n_guard) * sizeof(ohw_seam), hipMemcpyDeviceToHost));
}
}  // namespace
}  // namespace ohw

using namespace ohw;

extern "C" {

int ohw_stitch_plan_host(int64_t n_samples, int overlap_ms, int64_t* hop_samples, int64_t* n_windows) {
  return st_guard([&] {
    if (n_samples < 0) throw Error(OHW_E_INVALID_ARG, "stitch_plan: negative sample count");
    if (overlap_ms != 0 && (overlap_ms < 1000 || overlap_ms > 15000 || overlap_ms % 20 != 0))
      throw Error(OHW_E_INVALID_ARG, "stitch: the overlap is 0 (off) or a multiple of 20 ms in [1000, 15000], got " + std::to_string(overlap_ms));
    const int64_t H = (int64_t)CHUNK_SAMPLES - (int64_t)overlap_ms * 16;
    if (hop_samples) *hop_samples = H;
    if (n_windows) *n_windows = n_samples == 0 ? 0 : n_samples <= CHUNK_SAMPLES ? 1 : (n_samples - CHUNK_SAMPLES + H - 1) / H + 1;
  });
}

int ohw_stitch_seams_host(const int32_t* text_tokens, int stride, const int32_t* n_text, int n_windows, ohw_seam* seams_out) {
  return st_guard([&] {
    check_seam_args("stitch_seams_host", text_tokens, stride, n_text, n_windows, seams_out);
    for (int s = 0; s + 1 < n_windows; ++s) {
      const int32_t* left = text_tokens + (size_t)s * stride;
      const int32_t* right = text_tokens + (size_t)(s + 1) * stride;
      const int L = n_text[s], R = n_text[s + 1];
      SeamBest best{0.0, STITCH_NONE, 0};
      for (int i = 1; i <= L + R - 1; ++i) seam_take(best, seam_matches(left, L, right, R, i), i);
      seams_out[s] = seam_record(s, best, L, R);
    }
  });
}

int ohw_stitch_ranges_host(const ohw_seam* seams, const int32_t* n_text, int n_windows, int32_t* first_out, int32_t* end_out) {
  return st_guard([&] {
    if (n_windows < 0 || (n_windows > 0 && (!n_text || !first_out || !end_out)) || (n_windows > 1 && !seams))
      throw Error(OHW_E_INVALID_ARG, "stitch_ranges: bad argument");
    for (int w = 0; w < n_windows; ++w) {
      const int rc = w == 0 ? 0 : seams[w - 1].right_cut, lc = w + 1 == n_windows ? n_text[w] : seams[w].left_cut;
      first_out[w] = rc;
      end_out[w] = rc > lc ? rc : lc;
    }
  });
}

int ohw_stitch_clip_segment_host(const ohw_token_span* seg, int first, int end, float t_seam_left, float t_seam_right, ohw_token_span* out) {
  if (!seg || !out) return OHW_E_INVALID_ARG;
  if (seg->end <= first || seg->first >= end) return 0;
  auto clamp = [&](float t) { return t < seg->t0 ? seg->t0 : t > seg->t1 ? seg->t1 : t; };
  *out = *seg;
  if (seg->first < first) { out->first = first; out->t0 = clamp(t_seam_left); }
  if (seg->end > end) { out->end = end; out->t1 = clamp(t_seam_right); }
  return 1;
}

int ohw_stitch_seams(int device, const int32_t* text_tokens_host, int stride, const int32_t* n_text, int n_windows, ohw_seam* seams_out) {
  return st_guard([&] {
    check_seam_args("stitch_seams", text_tokens_host, stride, n_text, n_windows, seams_out);
    if (n_windows <= 1) return;
    stitch_device(device, text_tokens_host, stride, n_text, n_windows, 0, 0, seams_out);
  });
}

int ohw_dbg_stitch(int device, const int32_t* text_tokens_host, int stride, const int32_t* n_text, int n_windows, int n_guard, int32_t sentinel,
                   ohw_seam* seams_out) {
  return st_guard([&] {
    check_seam_args("dbg_stitch", text_tokens_host, stride, n_text, n_windows, seams_out);
    if (n_guard < 0 || n_guard > 1024) throw Error(OHW_E_INVALID_ARG, "dbg_stitch: 0 .. 1024 guard seams");
    if (n_windows <= 1) return;
    stitch_device(device, text_tokens_host, stride, n_text, n_windows, n_guard, sentinel, seams_out);
  });
}

}  // extern "C"
