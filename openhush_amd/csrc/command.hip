// command.hip — command lists: decoding constrained to listed phrases, on the device (include/ohw.h, ohw_state_set_command_table).
//
// The host compiles the phrases into an anchored flat trie (command_table_build_host); the kernel finds, per decoder row, the
// node whose path equals the text tokens of the row's own history, lowers every text column that is not a child of that node,
// and end-of-text unless a phrase ends there.  The host twin (command_rule_host) does the same single fp32 subtraction, so the
// two agree to the bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "kernels.hpp"

namespace ohw {
extern thread_local std::string g_last_error;                    // engine.hip

namespace {
template <typename F>
int cm_guard(F&& f) {
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
constexpr int CM_THREADS = 1024;
constexpr int CM_WAVES = CM_THREADS / 64;
constexpr int CM_LEN = OHW_PHRASE_MAX_LEN;
}  // namespace

void command_penalty_check(float penalty) {
  if (!(penalty > 0.f) || (penalty > OHW_COMMAND_PENALTY_MAX && !std::isinf(penalty)))       // false for NaN
    throw Error(OHW_E_INVALID_ARG, "command list: the penalty must lie in (0, 1000] or be +inf, got " + std::to_string(penalty));
}

// ---- the builder ---------------------------------------------------------------------------------------------------------
void command_table_build_host(const int32_t* tokens, const int32_t* offsets, int n_phrases, int eot, ohw_command_table* out) {
  if (!out || !out->child_off || !out->path || !out->child_tok || !out->terminal || !out->phrase_id)
    throw Error(OHW_E_INVALID_ARG, "command table: out and its five arrays are needed");
  if (n_phrases < 0 || n_phrases > OHW_PHRASE_MAX_PHRASES)
    throw Error(OHW_E_INVALID_ARG, "command table: " + std::to_string(n_phrases) + " phrases, at most " + std::to_string(OHW_PHRASE_MAX_PHRASES) + " fit");
  if (n_phrases > 0 && (!tokens || !offsets)) throw Error(OHW_E_INVALID_ARG, "command table: null argument");
  struct Node {
    std::set<int32_t> children;
    int32_t phrase = -1;
  };
  // per depth: path -> node; std::map orders the paths lexicographically, std::set the children by token
  std::vector<std::map<std::vector<int32_t>, Node>> level((size_t)CM_DEPTHS);
  for (int i = 0; i < n_phrases; ++i) {
    const std::string name = "command table: phrase " + std::to_string(i);
    const int64_t len = (int64_t)offsets[i + 1] - offsets[i];
    if (offsets[i] < 0 || len < 1 || len > CM_LEN)
      throw Error(OHW_E_INVALID_ARG, name + " has " + std::to_string(len) + " tokens, 1.." + std::to_string(CM_LEN) + " are allowed");
    const int32_t* t = tokens + offsets[i];
    for (int d = 0; d < (int)len; ++d)
      if (t[d] < 0 || t[d] >= eot)
        throw Error(OHW_E_INVALID_ARG, name + ": token " + std::to_string(t[d]) + " is not a text token (0 .. " + std::to_string(eot - 1) + ")");
    for (int d = 0; d <= (int)len; ++d) {
      Node& nd = level[(size_t)d][std::vector<int32_t>(t, t + d)];
      if (d < (int)len) nd.children.insert(t[d]);
      else if (nd.phrase < 0) nd.phrase = i;                       // phrases come in index order: the first is the lowest
    }
  }
  out->n_phrases = n_phrases;
  out->eot = eot;
  int node = 0, edge = 0, path = 0;
  for (int d = 0; d < CM_DEPTHS; ++d) {
    out->depth_start[d] = node;
    out->path_base[d] = path;
    for (const auto& kv : level[(size_t)d]) {
      std::memcpy(out->path + path, kv.first.data(), (size_t)d * 4);
      path += d;
      out->terminal[node] = kv.second.phrase >= 0;
      out->phrase_id[node] = kv.second.phrase;
      out->child_off[node++] = edge;
      for (int32_t c : kv.second.children) out->child_tok[edge++] = c;
    }
  }
  out->depth_start[CM_DEPTHS] = node;
  out->child_off[node] = edge;
  out->n_nodes = node; out->n_edges = edge; out->n_path = path;
}

namespace {
// every count and index of a table a caller hands in, before anything indexes with them
void command_table_check(const ohw_command_table* t) {
  if (!t || !t->child_off || !t->path || !t->child_tok || !t->terminal || !t->phrase_id) throw Error(OHW_E_INVALID_ARG, "command table: null table or array");
  bool ok = t->n_nodes >= 0 && t->n_nodes <= OHW_COMMAND_MAX_NODES && t->n_edges >= 0 && t->n_edges <= OHW_COMMAND_MAX_EDGES && t->n_path >= 0 &&
            t->n_path <= OHW_COMMAND_MAX_PATH && t->eot >= 0 && t->depth_start[0] == 0 && t->depth_start[CM_DEPTHS] == t->n_nodes;
  int path = 0;
  for (int d = 0; ok && d < CM_DEPTHS; ++d) {
    const int n = t->depth_start[d + 1] - t->depth_start[d];
    ok = n >= 0 && n <= OHW_PHRASE_MAX_PHRASES && t->path_base[d] == path;
    path += n * d;
  }
  ok = ok && path == t->n_path && t->child_off[0] == 0 && t->child_off[t->n_nodes] == t->n_edges && t->depth_start[1] <= 1;
  for (int n = 0; ok && n < t->n_nodes; ++n)
    ok = t->child_off[n + 1] >= t->child_off[n] && t->phrase_id[n] >= -1 && t->phrase_id[n] < OHW_PHRASE_MAX_PHRASES && (t->terminal[n] != 0) == (t->phrase_id[n] >= 0);
  for (int n = 0; ok && n < t->n_nodes; ++n)                      // children sorted and unique within a node: the marking pass relies on it
    for (int e = t->child_off[n]; ok && e < t->child_off[n + 1]; ++e)
      ok = t->child_tok[e] >= 0 && t->child_tok[e] < t->eot && (e == t->child_off[n] || t->child_tok[e] > t->child_tok[e - 1]);
  if (!ok) throw Error(OHW_E_INVALID_ARG, "command table: the arrays are not a table ohw_command_table_build_host made");
}

// the node whose path equals the entries of h[0 .. n) in [0, eot); -1: none (off the list).  *depth = the count of such entries
int command_node(const ohw_command_table* t, const int32_t* h, int n, int eot, int* depth) {
  int32_t text[CM_LEN];
  int d = 0;
  for (int i = 0; i < n; ++i) {
    if (h[i] < 0 || h[i] >= eot) continue;
    if (d < CM_LEN) text[d] = h[i];
    ++d;
  }
  *depth = d;
  if (d > CM_LEN) return -1;
  for (int nd = t->depth_start[d]; nd < t->depth_start[d + 1]; ++nd)
    if (d == 0 || std::memcmp(t->path + t->path_base[d] + (int64_t)(nd - t->depth_start[d]) * d, text, (size_t)d * 4) == 0) return nd;
  return -1;
}
}  // namespace

void command_rule_host(const ohw_command_table* t, float penalty, const int32_t* history, int n_cur, float* row, int n_vocab, int eot,
                       float* list_logprob_out) {
  command_penalty_check(penalty);
  command_table_check(t);
  if (n_cur < 0 || !row || n_vocab < 1 || eot < 0 || (n_cur > 0 && !history)) throw Error(OHW_E_INVALID_ARG, "command rule: bad history or row");
  const int lim = eot < n_vocab ? eot : n_vocab;                 // text tokens that have a column
  int d = 0;
  const int node = command_node(t, history, n_cur, eot, &d);
  std::vector<uint8_t> child((size_t)lim, 0);
  if (node >= 0)
    for (int e = t->child_off[node]; e < t->child_off[node + 1]; ++e)
      if (t->child_tok[e] < lim) child[(size_t)t->child_tok[e]] = 1;
  if (d == 0 && list_logprob_out) {
    auto lse = [&](bool only_children) {
      double m = -std::numeric_limits<double>::infinity(), s = 0.0;
      for (int c = 0; c < lim; ++c)
        if ((!only_children || child[(size_t)c]) && row[c] > m) m = row[c];
      if (std::isinf(m)) return m;
      for (int c = 0; c < lim; ++c)
        if ((!only_children || child[(size_t)c]) && !std::isinf(row[c])) s += std::exp((double)row[c] - m);
      return m + std::log(s);
    };
    const double lc = lse(true);
    *list_logprob_out = std::isinf(lc) ? -std::numeric_limits<float>::infinity() : (float)(lc - lse(false));
  }
  const bool hard = std::isinf(penalty);
  auto lower = [&](float x) { return hard ? OHW_REPEAT_BAN : x - penalty; };
  for (int c = 0; c < lim; ++c)
    if (!child[(size_t)c]) row[c] = lower(row[c]);
  if (node >= 0 && !t->terminal[node] && eot < n_vocab) row[eot] = lower(row[eot]);
}

int command_match_host(const ohw_command_table* t, const int32_t* tokens, int n) {
  command_table_check(t);
  if (n < 0 || (n > 0 && !tokens)) throw Error(OHW_E_INVALID_ARG, "command match: bad tokens");
  int d = 0;
  const int node = command_node(t, tokens, n, t->eot, &d);
  return node >= 0 ? t->phrase_id[node] : -1;
}

void command_table_pack(const ohw_command_table* t, float penalty, std::vector<int32_t>* words) {
  command_penalty_check(penalty);
  command_table_check(t);
  words->assign((size_t)CM_WORDS, 0);
  int32_t* w = words->data();
  std::memcpy(w + CM_OFF_DEPTH, t->depth_start, sizeof t->depth_start);
  std::memcpy(w + CM_OFF_BASE, t->path_base, sizeof t->path_base);
  std::memcpy(w + CM_OFF_PENALTY, &penalty, 4);
  std::memcpy(w + CM_OFF_CHILD, t->child_off, (size_t)(t->n_nodes + 1) * 4);
  std::memcpy(w + CM_OFF_TERM, t->terminal, (size_t)t->n_nodes * 4);
  std::memcpy(w + CM_OFF_PATH, t->path, (size_t)t->n_path * 4);
  std::memcpy(w + CM_OFF_TOK, t->child_tok, (size_t)t->n_edges * 4);
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------
// One workgroup of 16 waves per launch row (PhraseBoostParams' row mapping); a done row returns at once.
//   1. The history is compacted to its text tokens in LDS, 1024 positions a round (a ballot per wave, the waves' counts through
//      LDS); only the first 17 are kept, the count d decides the rest.
//   2. Wave 0 finds the depth-d node whose path equals them by phrase_boost_kernel's 64-way search over the depth's sorted
//      node range: a depth holds up to 1024 nodes, two rounds.
//   3. The node's children are marked in a bit map in LDS, one bit per text column.  The children are sorted, so those of one
//      map word are neighbours: the first of them gathers the word's bits and stores it, plainly - every word has one writer, no
//      atomics, and the writers of a wave hit different words.
//   4. One pass over the row's text columns: a lane reads its column and its map word (the 32 lanes of a half-wave read the
//      same word: a broadcast, no bank conflict) and stores x - p unless the bit is set.  Thread 0 lowers end-of-text.
// A window's first row whose history holds no text token also computes list_logprob: a pass for the two maxima ahead of 4, the
// two sums of expf(x - max) inside 4 (-inf columns enter neither), reduced over the lanes by shuffles and over the waves in LDS.
// Nothing at or behind tokens[n_cur] is read; columns above eot and guard columns are not touched.
__device__ __forceinline__ float cm_wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float cm_wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(CM_THREADS) void command_rule_kernel(CommandRuleParams p) {
  extern __shared__ uint32_t cm_bits[];                   // [(lim + 31) / 32]
  __shared__ int32_t text[CM_LEN + 1];
  __shared__ int32_t wave_cnt[CM_WAVES];
  __shared__ int32_t s_node;
  __shared__ float red[2][CM_WAVES];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = r * p.row_mul, win = h / p.group;
  if (p.done[win]) return;
  int n_cur = p.n_cur ? p.n_cur[win] : 0;
  n_cur = n_cur < 0 ? 0 : n_cur > p.max_tokens ? p.max_tokens : n_cur;
  const int32_t* depth_start = p.table + CM_OFF_DEPTH;
  const int32_t* path_base = p.table + CM_OFF_BASE;
  const int32_t* child_off = p.table + CM_OFF_CHILD;
  const int32_t* terminal = p.table + CM_OFF_TERM;
  const int32_t* path = p.table + CM_OFF_PATH;
  const int32_t* child_tok = p.table + CM_OFF_TOK;
  const float penalty = __int_as_float(p.table[CM_OFF_PENALTY]);
  const int lim = p.eot < p.n_vocab ? p.eot : p.n_vocab;  // text tokens that have a column
  const int n_words = (lim + 31) >> 5;
  for (int w = tid; w < n_words; w += CM_THREADS) cm_bits[w] = 0u;

  // 1. the text tokens of the history
  const int32_t* toks = p.tokens + (int64_t)h * p.max_tokens;
  int d = 0;                                              // uniform
  for (int base = 0; base < n_cur && d <= CM_LEN; base += CM_THREADS) {
    const int j = base + tid;
    const int t = j < n_cur ? toks[j] : -1;
    const bool is = (unsigned)t < (unsigned)p.eot;
    const unsigned long long b = __ballot(is);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int before = d, total = 0;
    for (int w = 0; w < CM_WAVES; ++w) {
      const int c = wave_cnt[w];
      if (w < wave) before += c;
      total += c;
    }
    const int pos = before + __popcll(b & ((1ull << lane) - 1ull));
    if (is && pos <= CM_LEN) text[pos] = t;
    d += total;
    __syncthreads();                                      // wave_cnt is written again in the next round
  }

  // 2. the node
  if (wave == 0) {
    int found = -1;
    if (d <= CM_LEN) {
      const int first = depth_start[d], end = depth_start[d + 1];
      if (first < end) {
        const int32_t* base = path + path_base[d];
        // lower bound of the text among the paths: the answer lies in [lo, hi]
        int lo = first, hi = end;
        while (lo < hi) {
          const int stride = (hi - lo + 63) / 64;
          const int n = lo + lane * stride;
          int cmp = 0;                                    // sign of (path of n) - text at their first difference
          if (n < hi) {
            const int32_t* q = base + (int64_t)(n - first) * d;
            for (int j = 0; j < d; ++j) {
              const int32_t a = q[j], c = text[j];
              if (cmp == 0) cmp = a < c ? -1 : a > c ? 1 : 0;
            }
          } else {
            cmp = 1;
          }
          const int c = __popcll(__ballot(cmp < 0));      // the paths are sorted: exactly the probes of lanes 0 .. c - 1 are below
          if (c == 0) { hi = lo; break; }
          const int below = lo + (c - 1) * stride;
          lo = below + 1;
          hi = below + stride < hi ? below + stride : hi;
        }
        if (lo < end) {
          const int32_t* q = base + (int64_t)(lo - first) * d;
          const bool same = lane >= d || q[lane] == text[lane];      // one lane per token of the candidate's path
          if (__all(same)) found = lo;
        }
      }
    }
    if (lane == 0) s_node = found;
  }
  __syncthreads();                                        // also: the bit map is zero, text is whole
  const int node = s_node;

  // 3. the children's bits
  if (node >= 0) {
    const int e0 = child_off[node], e1 = child_off[node + 1];
    for (int e = e0 + tid; e < e1; e += CM_THREADS) {
      const int t = child_tok[e], w = t >> 5;
      if ((unsigned)t >= (unsigned)lim) continue;         // a child without a column
      if (e > e0 && (child_tok[e - 1] >> 5) == w) continue;          // not the first child of its word
      uint32_t bits = 0u;
      for (int k = e; k < e1; ++k) {
        const int tk = child_tok[k];
        if ((tk >> 5) != w) break;
        if (tk < lim) bits |= 1u << (tk & 31);
      }
      cm_bits[w] = bits;
    }
  }
  __syncthreads();

  float* row = p.logits + (int64_t)r * p.ld;
  const bool hard = isinf(penalty);
  const bool lp = d == 0 && p.list_logprob && h % p.lp_group == 0;   // uniform
  float m_all = -INFINITY, m_ch = -INFINITY;
  if (lp) {
    for (int c = tid; c < lim; c += CM_THREADS) {
      const float x = row[c];
      m_all = fmaxf(m_all, x);
      if ((cm_bits[c >> 5] >> (c & 31)) & 1u) m_ch = fmaxf(m_ch, x);
    }
    m_all = cm_wave_max(m_all); m_ch = cm_wave_max(m_ch);
    if (lane == 0) { red[0][wave] = m_all; red[1][wave] = m_ch; }
    __syncthreads();
    m_all = red[0][0]; m_ch = red[1][0];
    for (int w = 1; w < CM_WAVES; ++w) { m_all = fmaxf(m_all, red[0][w]); m_ch = fmaxf(m_ch, red[1][w]); }
    __syncthreads();                                      // red is written again below
  }

  // 4. the row
  float s_all = 0.f, s_ch = 0.f;
  for (int c = tid; c < lim; c += CM_THREADS) {
    const float x = row[c];
    const bool child = (cm_bits[c >> 5] >> (c & 31)) & 1u;
    if (lp && x > -INFINITY) {
      s_all += expf(x - m_all);
      if (child) s_ch += expf(x - m_ch);
    }
    if (!child) row[c] = hard ? OHW_REPEAT_BAN : x - penalty;
  }
  if (tid == 0 && node >= 0 && !terminal[node] && p.eot < p.n_vocab) {
    const float x = row[p.eot];
    row[p.eot] = hard ? OHW_REPEAT_BAN : x - penalty;
  }
  if (lp) {
    s_all = cm_wave_sum(s_all); s_ch = cm_wave_sum(s_ch);
    if (lane == 0) { red[0][wave] = s_all; red[1][wave] = s_ch; }
    __syncthreads();
    if (tid == 0) {
      s_all = red[0][0]; s_ch = red[1][0];
      for (int w = 1; w < CM_WAVES; ++w) { s_all += red[0][w]; s_ch += red[1][w]; }
      p.list_logprob[h / p.lp_group] = s_ch > 0.f ? (m_ch + logf(s_ch)) - (m_all + logf(s_all)) : -INFINITY;
    }
  }
}

void launch_command_rule(const CommandRuleParams& p, int rows, hipStream_t s) {
  if (rows < 1 || !p.logits || !p.tokens || !p.done || !p.table || p.row_mul < 1 || p.group < 1 || p.lp_group < 1 || p.n_vocab < 1 || p.n_vocab > p.ld ||
      p.n_vocab > CM_MAX_VOCAB || p.max_tokens < 1 || p.eot < 0)
    throw Error(OHW_E_INVALID_ARG, "command rule: bad launch");
  const int lim = p.eot < p.n_vocab ? p.eot : p.n_vocab;
  hipLaunchKernelGGL(command_rule_kernel, dim3(rows), dim3(CM_THREADS), (size_t)((lim + 31) / 32 + 1) * 4, s, p);
  HIP_CHECK(hipGetLastError());
}

}  // namespace ohw

using namespace ohw;

extern "C" {

int ohw_command_table_build_host(const int32_t* tokens, const int32_t* offsets, int n_phrases, int eot, ohw_command_table* out) {
  return cm_guard([&] { command_table_build_host(tokens, offsets, n_phrases, eot, out); });
}

int ohw_command_rule_host(const ohw_command_table* table, float penalty, const int32_t* history, int n_cur, float* row, int n_vocab, int eot,
                          float* list_logprob_out) {
  return cm_guard([&] { command_rule_host(table, penalty, history, n_cur, row, n_vocab, eot, list_logprob_out); });
}

int ohw_command_match_host(const ohw_command_table* table, const int32_t* tokens, int n) {
  int id = -1;
  const int rc = cm_guard([&] { id = command_match_host(table, tokens, n); });
  return rc == OHW_OK ? id : -1;
}

}  // extern "C"
