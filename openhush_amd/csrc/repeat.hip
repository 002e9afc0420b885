// repeat.hip — repetition penalty and no-repeat n-grams on the device (include/ohw.h, ohw_state_set_repeat_rule).
//
// Per decoder row, on the row's own sampled tokens: every distinct text token of the history has its logit scaled away from the
// sampler (x < 0 ? x * theta : x / theta), then every text token that would complete an n-gram the history already holds is set to
// OHW_REPEAT_BAN.  The host twin (repeat_rule_host) does the same fp32 arithmetic, so the two agree to the bit.
#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "kernels.hpp"

namespace ohw {
extern thread_local std::string g_last_error;                    // engine.hip

namespace {
constexpr int RP_THREADS = 256;
constexpr int RP_MAX_TOKENS = 4096;      // the history and the loaded logits live in LDS: 2 * 4 bytes per position, 32 KiB at most
}  // namespace

void repeat_rule_check(float penalty, int ngram) {
  if (!(penalty >= OHW_REPEAT_PENALTY_MIN && penalty <= OHW_REPEAT_PENALTY_MAX))      // false for NaN
    throw Error(OHW_E_INVALID_ARG, "repeat rule: the penalty must lie in [0.01, 100], got " + std::to_string(penalty));
  if (ngram < 0 || ngram > OHW_REPEAT_MAX_NGRAM)
    throw Error(OHW_E_INVALID_ARG, "repeat rule: the n-gram size must lie in [0, 32], got " + std::to_string(ngram));
}

void repeat_rule_host(float penalty, int ngram, const int32_t* history, int n_cur, float* row, int n_vocab, int eot) {
  repeat_rule_check(penalty, ngram);
  if (n_cur < 0 || !row || n_vocab < 1 || eot < 0 || (n_cur > 0 && !history)) throw Error(OHW_E_INVALID_ARG, "repeat rule: bad history or row");
  const int lim = eot < n_vocab ? eot : n_vocab;                 // text tokens that have a column
  auto text = [&](int32_t t) { return t >= 0 && t < lim; };
  if (penalty != 1.0f) {
    std::vector<int32_t> seen;
    for (int i = 0; i < n_cur; ++i) if (text(history[i])) seen.push_back(history[i]);
    std::sort(seen.begin(), seen.end());
    seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
    for (int32_t t : seen) {
      const float x = row[t];
      row[t] = x < 0.f ? x * penalty : x / penalty;
    }
  }
  if (ngram >= 1 && n_cur >= ngram) {                            // a start needs 0 <= i <= n_cur - n
    const int m = ngram - 1;                                     // the tail's length
    const int32_t* tail = history + (n_cur - m);
    for (int i = 0; i + ngram <= n_cur; ++i) {
      if (!std::equal(history + i, history + i + m, tail)) continue;
      const int32_t f = history[i + m];
      if (text(f)) row[f] = OHW_REPEAT_BAN;
    }
  }
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------
// One workgroup per launch row (PhraseBoostParams' row mapping).  The row's history goes to LDS in one round trip; everything
// after that reads it there.  One thread per history position, strided, so a history longer than the workgroup is covered.
// Penalty: every position of a text token loads the token's logit, ALL positions' loads end at a barrier, then every position
// stores the scaled value.  The positions of one token have loaded the same word and store the same word, so the token is
// scaled once however often it occurs, with no atomics and no search for a first or last occurrence: one load and one store per
// position, none of them dependent on another.
// Ban, behind a second barrier so that it lands after the penalty: position q is a follower when the n - 1 tokens in front of
// it equal the history's last n - 1 (compared in LDS, raw ids); a text follower's logit becomes OHW_REPEAT_BAN.  The stores are
// plain and all write the same value.
// Nothing at or behind tokens[n_cur] is read; done rows, columns >= n_vocab and non-text tokens' columns are not touched.
__global__ __launch_bounds__(RP_THREADS) void repeat_rule_kernel(RepeatRuleParams p) {
  extern __shared__ int32_t rp_lds[];                     // hist [max_tokens], then the loaded logits [max_tokens]
  const int r = blockIdx.x, tid = threadIdx.x;
  const int h = r * p.row_mul, win = h / p.group;
  // the four uniform words in ONE round trip: all four scalar loads are issued before the first is looked at (the empty asm
  // keeps the compiler from sinking a load behind the branch on another's value); a null n_cur loads the done word again
  const int dn = p.done[win];
  const int nc = *(p.n_cur ? p.n_cur + win : p.done + win);
  const int theta_bits = p.rule[0], n = p.rule[1];
  asm volatile("" ::"s"(dn), "s"(nc), "s"(theta_bits), "s"(n));
  int n_cur = p.n_cur ? nc : 0;
  const float theta = __int_as_float(theta_bits);
  if (dn || n_cur <= 0) return;
  if (n_cur > p.max_tokens) n_cur = p.max_tokens;         // the LDS arrays' size
  int32_t* hist = rp_lds;
  float* xs = (float*)(rp_lds + p.max_tokens);
  const int lim = p.eot < p.n_vocab ? p.eot : p.n_vocab;  // text tokens that have a column
  const int32_t* toks = p.tokens + (int64_t)h * p.max_tokens;
  float* row = p.logits + (int64_t)r * p.ld;
  for (int j = tid; j < n_cur; j += RP_THREADS) hist[j] = toks[j];
  __syncthreads();
  if (theta != 1.0f) {                                    // uniform: the barrier inside is reached by all threads or by none
    for (int j = tid; j < n_cur; j += RP_THREADS) {
      const int t = hist[j];
      if ((unsigned)t < (unsigned)lim) xs[j] = row[t];
    }
    __syncthreads();                                      // every load of the row is done before any store to it
    for (int j = tid; j < n_cur; j += RP_THREADS) {
      const int t = hist[j];
      if ((unsigned)t < (unsigned)lim) {
        const float x = xs[j];                            // this thread's own word
        row[t] = x < 0.f ? x * theta : x / theta;
      }
    }
  }
  if (n < 1 || n > n_cur) return;                         // uniform; n > n_cur: no start 0 <= i <= n_cur - n
  __syncthreads();                                        // the ban lands after the penalty
  const int m = n - 1;
  const int32_t* tail = hist + (n_cur - m);
  for (int q = m + tid; q < n_cur; q += RP_THREADS) {     // q = i + n - 1 for the start i = q - m in 0 .. n_cur - n
    const int f = hist[q];
    if ((unsigned)f >= (unsigned)lim) continue;           // only text tokens are ever banned
    const int32_t* g = hist + (q - m);
    bool same = true;
    for (int k = 0; k < m && same; ++k) same = g[k] == tail[k];
    if (same) row[f] = OHW_REPEAT_BAN;
  }
}

void launch_repeat_rule(const RepeatRuleParams& p, int rows, hipStream_t s) {
  if (rows < 1 || !p.logits || !p.tokens || !p.done || !p.rule || p.row_mul < 1 || p.group < 1 || p.n_vocab < 1 || p.n_vocab > p.ld || p.max_tokens < 1 ||
      p.max_tokens > RP_MAX_TOKENS || p.eot < 0)
    throw Error(OHW_E_INVALID_ARG, "repeat rule: bad launch");
  hipLaunchKernelGGL(repeat_rule_kernel, dim3(rows), dim3(RP_THREADS), (size_t)p.max_tokens * 8, s, p);
  HIP_CHECK(hipGetLastError());
}

}  // namespace ohw

using namespace ohw;

extern "C" {

int ohw_repeat_rule_host(float penalty, int ngram, const int32_t* history, int n_cur, float* row, int n_vocab, int eot) {
  try {
    repeat_rule_host(penalty, ngram, history, n_cur, row, n_vocab, eot);
    return OHW_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "host allocation failed";
    return OHW_E_OOM;
  }
}

}  // extern "C"
