// score.hip — confidence: the five words of a logits row a host needs (include/ohw.h, ohw_token_score / ohw_state_score).
//
// token_score_kernel reduces one raw fp32 logits row per workgroup to {x[target], log-sum-exp over the text columns, log-sum-exp
// over all columns, the first arg-max among the text columns, its value}.  The host twin (ohw_token_score_host) walks the same
// columns through the same fp32 operations in the same order, so the selections agree word for word; the two log-sum-exp values
// differ only by what expf / logf differ between the two libraries (tests/score_ref.py derives the bound from the order below).
//
// THE REDUCTION ORDER (a function of n_vocab and eot alone - never of the batch, the row's slot or the CUs):
//   1. TS_THREADS = 256 threads.  Thread t takes the 16-byte groups g = t, t + 256, t + 512 ... below ceil(n_vocab / 4), in that
//      order, and in a group the columns c = 4 g .. 4 g + 3 in ascending order.  A column c >= n_vocab is loaded (it lies inside
//      the row's ld) and dropped.  A column c < eot updates the thread's TEXT pair and its arg-max (strictly greater wins: the first
//      maximum of the thread), a column eot <= c < n_vocab its SPECIAL pair.  A pair (m, s) starts at (-inf, 0); a column x
//      makes it   mn = max(m, x);  s = s * exp(m - mn) + exp(x - mn);  m = mn   (no fused multiply-add).
//   2. The 64 lanes of a wave: an xor tree, offsets 32, 16, 8, 4, 2, 1; a step makes of the lane's own pair (m1, s1) and the
//      partner's (m2, s2):   mn = max(m1, m2);  s = mn == -inf ? 0 : s1 * exp(m1 - mn) + s2 * exp(m2 - mn).  The sum is
//      commutative and nothing is fused, so every lane of a wave ends with the same words.  The arg-max takes the greater
//      value, and on equal values the smaller column.
//   3. The 4 waves: wave 0's result, then waves 1, 2, 3 folded in with the same step, in that order.
//   4. lse_text = m_text + log(s_text);  (m_all, s_all) = the step on (text, special);  lse_all = m_all + log(s_all).
//   logit = x[target] is one load of its own.
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "kernels.hpp"

namespace ohw {
extern thread_local std::string g_last_error;                    // engine.hip

namespace {
template <typename F>
int sc_guard(F&& f) {
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
constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / 64;

struct Pair { float m, s; };
struct Best { float v; int32_t i; };

// one column into a running pair; one pair into another.  Host and device: the same source, contraction off
__host__ __device__ __forceinline__ void pair_add(Pair& a, float x) {
#pragma clang fp contract(off)
  const float mn = fmaxf(a.m, x);
  const float e0 = expf(a.m - mn), e1 = expf(x - mn);
  const float t = a.s * e0;
  a.s = t + e1;
  a.m = mn;
}
__host__ __device__ __forceinline__ Pair pair_merge(const Pair& a, const Pair& b) {
#pragma clang fp contract(off)
  const float mn = fmaxf(a.m, b.m);
  Pair r{mn, 0.f};
  if (mn != -INFINITY) {
    const float t0 = a.s * expf(a.m - mn), t1 = b.s * expf(b.m - mn);
    r.s = t0 + t1;
  }
  return r;
}
__host__ __device__ __forceinline__ Best best_merge(const Best& a, const Best& b) {
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__host__ __device__ __forceinline__ void score_finish(const Pair& text, const Pair& special, const Best& best, float logit, ohw_token_score* out) {
#pragma clang fp contract(off)
  const Pair all = pair_merge(text, special);
  out->logit = logit;
  out->lse_text = text.m + logf(text.s);
  out->lse_all = all.m + logf(all.s);
  out->top_id = best.i == INT32_MAX ? 0 : best.i;
  out->top_logit = best.v;
}

__global__ __launch_bounds__(TS_THREADS) void token_score_kernel(TokenScoreParams p) {
  const int m = blockIdx.x, b = m >> 3, pos = p.row0 + (m & 7);
  const int entry = pos - (p.n_prompt - 1);
  if (entry < 0 || entry >= p.cap || pos >= p.n_all[b]) return;          // the whole workgroup: nothing of this row is read or written
  const float* __restrict__ x = p.logits + (int64_t)m * p.ld;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_vocab = p.n_vocab, eot = p.eot < n_vocab ? p.eot : n_vocab;
  const int groups = (n_vocab + 3) >> 2;                                  // 4 * groups <= ld: the launcher checks it
  Pair text{-INFINITY, 0.f}, special{-INFINITY, 0.f};
  Best best{-INFINITY, INT32_MAX};
  for (int g = tid; g < groups; g += TS_THREADS) {
    const f32x4 q = *(const f32x4*)(x + 4 * (int64_t)g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = 4 * g + r;
      const float v = q[r];
      if (c < eot) {
        pair_add(text, v);
        if (v > best.v) best = Best{v, c};
      } else if (c < n_vocab) {
        pair_add(special, v);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const Pair to{__shfl_xor(text.m, o, 64), __shfl_xor(text.s, o, 64)};
    const Pair so{__shfl_xor(special.m, o, 64), __shfl_xor(special.s, o, 64)};
    const Best bo{__shfl_xor(best.v, o, 64), __shfl_xor(best.i, o, 64)};
    text = pair_merge(text, to);
    special = pair_merge(special, so);
    best = best_merge(best, bo);
  }
  __shared__ float w_f[TS_WAVES][5];
  __shared__ int32_t w_i[TS_WAVES];
  if (lane == 0) {
    w_f[wave][0] = text.m; w_f[wave][1] = text.s; w_f[wave][2] = special.m; w_f[wave][3] = special.s; w_f[wave][4] = best.v;
    w_i[wave] = best.i;
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int w = 1; w < TS_WAVES; ++w) {
    text = pair_merge(text, Pair{w_f[w][0], w_f[w][1]});
    special = pair_merge(special, Pair{w_f[w][2], w_f[w][3]});
    best = best_merge(best, Best{w_f[w][4], w_i[w]});
  }
  const int target = p.targets[m];
  const float logit = (target >= 0 && target < n_vocab) ? x[target] : -INFINITY;
  score_finish(text, special, best, logit, p.out + (int64_t)b * p.cap + entry);
}
}  // namespace

void launch_token_score(const TokenScoreParams& p, hipStream_t s) {
  if (!p.logits || !p.targets || !p.n_all || !p.out || p.batch < 1 || p.n_vocab < 1 || p.eot < 0 || p.cap < 1 || p.n_prompt < 1 || p.row0 < 0)
    throw Error(OHW_E_INVALID_ARG, "token_score: null buffer or bad shape");
  if (p.ld % 4 != 0 || p.ld < p.n_vocab || ((uintptr_t)p.logits & 15) != 0)
    throw Error(OHW_E_INVALID_ARG, "token_score: the rows are read 16 bytes at a time: ld % 4 == 0, ld >= n_vocab, a 16-byte aligned base");
  hipLaunchKernelGGL(token_score_kernel, dim3(p.batch * 8), dim3(TS_THREADS), 0, s, p);
  HIP_CHECK(hipGetLastError());
}

// the rule on the host: the order of the header comment, thread by thread, lane by lane, wave by wave
void token_score_host(const float* x, int n_vocab, int eot_in, int target, ohw_token_score* out) {
  if (!x || !out || n_vocab < 1 || eot_in < 0) throw Error(OHW_E_INVALID_ARG, "token_score_host: null argument or bad shape");
  const int eot = eot_in < n_vocab ? eot_in : n_vocab, groups = (n_vocab + 3) >> 2;
  std::vector<Pair> text((size_t)TS_THREADS, Pair{-INFINITY, 0.f}), special((size_t)TS_THREADS, Pair{-INFINITY, 0.f});
  std::vector<Best> best((size_t)TS_THREADS, Best{-INFINITY, INT32_MAX});
  for (int t = 0; t < TS_THREADS; ++t)
    for (int g = t; g < groups; g += TS_THREADS)
      for (int r = 0; r < 4; ++r) {
        const int c = 4 * g + r;
        if (c < eot) {
          pair_add(text[(size_t)t], x[c]);
          if (x[c] > best[(size_t)t].v) best[(size_t)t] = Best{x[c], c};
        } else if (c < n_vocab) {
          pair_add(special[(size_t)t], x[c]);
        }
      }
  for (int o = 32; o > 0; o >>= 1) {
    const std::vector<Pair> t0 = text, s0 = special;
    const std::vector<Best> b0 = best;
    for (int t = 0; t < TS_THREADS; ++t) {
      const size_t q = (size_t)((t & ~63) | ((t & 63) ^ o));
      text[(size_t)t] = pair_merge(t0[(size_t)t], t0[q]);
      special[(size_t)t] = pair_merge(s0[(size_t)t], s0[q]);
      best[(size_t)t] = best_merge(b0[(size_t)t], b0[q]);
    }
  }
  Pair tx = text[0], sp = special[0];
  Best bs = best[0];
  for (int w = 1; w < TS_WAVES; ++w) {
    tx = pair_merge(tx, text[(size_t)w * 64]);
    sp = pair_merge(sp, special[(size_t)w * 64]);
    bs = best_merge(bs, best[(size_t)w * 64]);
  }
  score_finish(tx, sp, bs, (target >= 0 && target < n_vocab) ? x[target] : -INFINITY, out);
}

}  // namespace ohw

extern "C" {
int ohw_token_score_host(const float* x, int n_vocab, int eot, int target, ohw_token_score* out) {
  return ohw::sc_guard([&] { ohw::token_score_host(x, n_vocab, eot, target, out); });
}

int ohw_token_prob_host(const ohw_token_score* s, float* logprob_text, float* logprob_all, float* top_logprob_text) {
  return ohw::sc_guard([&] {
    if (!s) throw ohw::Error(OHW_E_INVALID_ARG, "token_prob_host: null score");
    if (logprob_text) *logprob_text = s->logit - s->lse_text;
    if (logprob_all) *logprob_all = s->logit - s->lse_all;
    if (top_logprob_text) *top_logprob_text = s->top_logit - s->lse_text;
  });
}

int ohw_word_probs_host(const float* logprob_text, const int32_t* starts, int n, float* probs_out) {
  int words = 0;
  const int rc = ohw::sc_guard([&] {
    if (n < 0 || (n > 0 && (!logprob_text || !starts || !probs_out))) throw ohw::Error(OHW_E_INVALID_ARG, "word_probs_host: null argument or n < 0");
    double sum = 0.0;
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
      if (i > 0 && starts[i]) {               // token 0 always opens the window's first word
        probs_out[words++] = (float)(sum / cnt);
        sum = 0.0; cnt = 0;
      }
      sum += std::exp((double)logprob_text[i]);
      ++cnt;
    }
    if (cnt > 0) probs_out[words++] = (float)(sum / cnt);
  });
  return rc == OHW_OK ? words : rc;
}
}  // extern "C"
