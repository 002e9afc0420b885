// phrase.hip — hot phrases: a history-dependent logit boost on the device (include/ohw.h, ohw_state_set_phrase_table).
//
// The host compiles the phrases into a flat trie (phrase_table_build_host); the kernel finds, per decoder row, the node of
// every depth whose path equals the tail of the row's own history, and adds the boosts of those nodes' children to the row, in
// table order.  The host twin (phrase_boost_host) runs the same fp32 adds in the same order, so the two agree to the bit.
#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "kernels.hpp"

namespace ohw {
extern thread_local std::string g_last_error;                    // engine.hip

namespace {
template <typename F>
int ph_guard(F&& f) {
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
constexpr int PH_THREADS = 256;
constexpr int PH_TAIL = OHW_PHRASE_MAX_LEN - 1;      // the deepest node's path: 15 tokens
}  // namespace

// ---- the builder ---------------------------------------------------------------------------------------------------------
void phrase_table_build_host(const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases, int eot, ohw_phrase_table* out) {
  if (!out || !out->child_off || !out->path || !out->child_tok || !out->child_boost) throw Error(OHW_E_INVALID_ARG, "phrase table: out and its four arrays are needed");
  if (n_phrases < 0 || n_phrases > OHW_PHRASE_MAX_PHRASES)
    throw Error(OHW_E_INVALID_ARG, "phrase table: " + std::to_string(n_phrases) + " phrases, at most " + std::to_string(OHW_PHRASE_MAX_PHRASES) + " fit");
  if (n_phrases > 0 && (!tokens || !offsets || !boosts)) throw Error(OHW_E_INVALID_ARG, "phrase table: null argument");
  // per depth: path -> (token -> boost); std::map orders the paths lexicographically and the children by token
  using Children = std::map<int32_t, float>;
  std::vector<std::map<std::vector<int32_t>, Children>> level((size_t)OHW_PHRASE_MAX_LEN);
  for (int i = 0; i < n_phrases; ++i) {
    const std::string name = "phrase table: phrase " + std::to_string(i);
    const int64_t len = (int64_t)offsets[i + 1] - offsets[i];
    if (offsets[i] < 0 || len < 1 || len > OHW_PHRASE_MAX_LEN)
      throw Error(OHW_E_INVALID_ARG, name + " has " + std::to_string(len) + " tokens, 1.." + std::to_string(OHW_PHRASE_MAX_LEN) + " are allowed");
    if (!std::isfinite(boosts[i])) throw Error(OHW_E_INVALID_ARG, name + " has a boost that is not finite");
    const int32_t* t = tokens + offsets[i];
    for (int d = 0; d < (int)len; ++d)
      if (t[d] < 0 || t[d] >= eot)
        throw Error(OHW_E_INVALID_ARG, name + ": token " + std::to_string(t[d]) + " is not a text token (0 .. " + std::to_string(eot - 1) + ")");
    for (int d = 0; d < (int)len; ++d) {
      Children& ch = level[(size_t)d][std::vector<int32_t>(t, t + d)];
      auto it = ch.find(t[d]);
      if (it == ch.end()) ch.emplace(t[d], boosts[i]);
      else if (boosts[i] > it->second) it->second = boosts[i];      // an edge's boost: the maximum over its phrases
    }
  }
  out->n_phrases = n_phrases;
  int node = 0, edge = 0, path = 0;
  for (int d = 0; d < OHW_PHRASE_MAX_LEN; ++d) {
    out->depth_start[d] = node;
    out->path_base[d] = path;
    for (const auto& kv : level[(size_t)d]) {
      std::memcpy(out->path + path, kv.first.data(), (size_t)d * 4);
      path += d;
      out->child_off[node++] = edge;
      for (const auto& c : kv.second) { out->child_tok[edge] = c.first; out->child_boost[edge] = c.second; ++edge; }
    }
  }
  out->depth_start[OHW_PHRASE_MAX_LEN] = node;
  out->child_off[node] = edge;
  out->n_nodes = node; out->n_edges = edge; out->n_path = path;
}

namespace {
// every count and index of a table a caller hands in, before anything indexes with them
void phrase_table_check(const ohw_phrase_table* t, int n_vocab) {
  if (!t || !t->child_off || !t->path || !t->child_tok || !t->child_boost) throw Error(OHW_E_INVALID_ARG, "phrase table: null table or array");
  bool ok = t->n_nodes >= 0 && t->n_nodes <= OHW_PHRASE_MAX_NODES && t->n_edges >= 0 && t->n_edges <= OHW_PHRASE_MAX_EDGES && t->n_path >= 0 &&
            t->n_path <= OHW_PHRASE_MAX_PATH && t->depth_start[0] == 0 && t->depth_start[OHW_PHRASE_MAX_LEN] == t->n_nodes;
  int path = 0;
  for (int d = 0; ok && d < OHW_PHRASE_MAX_LEN; ++d) {
    const int n = t->depth_start[d + 1] - t->depth_start[d];
    ok = n >= 0 && t->path_base[d] == path;
    path += n * d;
  }
  ok = ok && path == t->n_path && t->child_off[0] == 0 && t->child_off[t->n_nodes] == t->n_edges;
  for (int n = 0; ok && n < t->n_nodes; ++n) ok = t->child_off[n + 1] >= t->child_off[n];
  for (int e = 0; ok && e < t->n_edges; ++e) ok = t->child_tok[e] >= 0 && t->child_tok[e] < n_vocab;
  if (!ok) throw Error(OHW_E_INVALID_ARG, "phrase table: the arrays are not a table ohw_phrase_table_build_host made for this vocabulary");
}
}  // namespace

void phrase_boost_host(const ohw_phrase_table* t, const int32_t* history, int n_cur, float* row, int n_vocab) {
  phrase_table_check(t, n_vocab);
  if (n_cur < 0 || !row || (n_cur > 0 && !history)) throw Error(OHW_E_INVALID_ARG, "phrase boost: bad history or row");
  for (int d = 0; d < OHW_PHRASE_MAX_LEN && d <= n_cur; ++d) {
    const int32_t* tail = history + (n_cur - d);
    for (int n = t->depth_start[d]; n < t->depth_start[d + 1]; ++n) {
      if (d > 0 && std::memcmp(t->path + t->path_base[d] + (int64_t)(n - t->depth_start[d]) * d, tail, (size_t)d * 4) != 0) continue;
      for (int e = t->child_off[n]; e < t->child_off[n + 1]; ++e) row[t->child_tok[e]] = row[t->child_tok[e]] + t->child_boost[e];
      break;     // paths are unique within a depth
    }
  }
}

void phrase_table_pack(const ohw_phrase_table* t, int n_vocab, std::vector<int32_t>* words) {
  phrase_table_check(t, n_vocab);
  words->assign((size_t)PH_WORDS, 0);
  int32_t* w = words->data();
  std::memcpy(w + PH_OFF_DEPTH, t->depth_start, sizeof t->depth_start);
  std::memcpy(w + PH_OFF_BASE, t->path_base, sizeof t->path_base);
  std::memcpy(w + PH_OFF_CHILD, t->child_off, (size_t)(t->n_nodes + 1) * 4);
  std::memcpy(w + PH_OFF_PATH, t->path, (size_t)t->n_path * 4);
  std::memcpy(w + PH_OFF_TOK, t->child_tok, (size_t)t->n_edges * 4);
  std::memcpy(w + PH_OFF_BOOST, t->child_boost, (size_t)t->n_edges * 4);
}

// ---- the kernel ----------------------------------------------------------------------------------------------------------
// One workgroup of 4 waves per launch row.  The last 15 history tokens go to LDS; wave v takes depths v, v + 4, ... and finds
// the depth's node whose path equals the history's tail by a 64-way search over the depth's sorted node range (every lane
// compares one probe node, the ballot's count narrows the range: two rounds for 1024 nodes).  Then, depth by depth, all
// threads stride over the matched node's children with plain load - add - store (tokens are unique within a node) and a
// barrier between nodes, which orders the adds of nested matches as the host twin orders them.
__global__ __launch_bounds__(PH_THREADS) void phrase_boost_kernel(PhraseBoostParams p) {
  __shared__ int32_t tail[PH_TAIL];                       // tail[PH_TAIL - 1] = the newest token
  __shared__ int32_t matched[OHW_PHRASE_MAX_LEN];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = r * p.row_mul, win = h / p.group;
  if (p.done[win]) return;
  const int n_cur = p.n_cur ? p.n_cur[win] : 0;
  const int32_t* depth_start = p.table + PH_OFF_DEPTH;
  const int32_t* path_base = p.table + PH_OFF_BASE;
  const int32_t* child_off = p.table + PH_OFF_CHILD;
  const int32_t* path = p.table + PH_OFF_PATH;
  const int32_t* child_tok = p.table + PH_OFF_TOK;
  const float* child_boost = (const float*)(p.table + PH_OFF_BOOST);
  if (tid < PH_TAIL) {
    const int i = n_cur - PH_TAIL + tid;                  // < n_cur: nothing at or behind tokens[n_cur] is read
    tail[tid] = i >= 0 ? p.tokens[(int64_t)h * p.max_tokens + i] : -1;
  }
  __syncthreads();
  for (int d = wave; d < OHW_PHRASE_MAX_LEN; d += PH_THREADS / 64) {
    const int first = depth_start[d], end = depth_start[d + 1];
    int found = -1;
    if (d <= n_cur && first < end) {
      const int32_t* base = path + path_base[d];
      const int32_t* want = tail + (PH_TAIL - d);
      // lower bound of the tail among the paths: the answer lies in [lo, hi]
      int lo = first, hi = end;
      while (lo < hi) {
        const int stride = (hi - lo + 63) / 64;
        const int n = lo + lane * stride;
        int cmp = 0;                                      // sign of (path of n) - tail at their first difference
        if (n < hi) {
          const int32_t* q = base + (int64_t)(n - first) * d;
          for (int j = 0; j < d; ++j) {
            const int32_t a = q[j], b = want[j];
            if (cmp == 0) cmp = a < b ? -1 : a > b ? 1 : 0;
          }
        } else {
          cmp = 1;
        }
        const int c = __popcll(__ballot(cmp < 0));        // the paths are sorted: exactly the probes of lanes 0 .. c - 1 are below
        if (c == 0) { hi = lo; break; }
        const int below = lo + (c - 1) * stride;
        lo = below + 1;
        hi = below + stride < hi ? below + stride : hi;
      }
      if (lo < end) {
        // one lane per token of the candidate's path
        const int32_t* q = base + (int64_t)(lo - first) * d;
        const bool same = lane >= d || q[lane] == want[lane];
        if (__all(same)) found = lo;
      }
    }
    if (lane == 0) matched[d] = found;
  }
  __syncthreads();
  float* row = p.logits + (int64_t)r * p.ld;
  for (int d = 0; d < OHW_PHRASE_MAX_LEN; ++d) {
    const int n = matched[d];                             // uniform over the workgroup
    if (n < 0) continue;
    const int e1 = child_off[n + 1];
    for (int e = child_off[n] + tid; e < e1; e += PH_THREADS) {
      const int t = child_tok[e];
      if ((unsigned)t < (unsigned)p.n_vocab) row[t] = row[t] + child_boost[e];
    }
    __syncthreads();
  }
}

void launch_phrase_boost(const PhraseBoostParams& p, int rows, hipStream_t s) {
  if (rows < 1 || !p.logits || !p.tokens || !p.done || !p.table || p.row_mul < 1 || p.group < 1 || p.n_vocab < 1 || p.n_vocab > p.ld || p.max_tokens < 1)
    throw Error(OHW_E_INVALID_ARG, "phrase boost: bad launch");
  hipLaunchKernelGGL(phrase_boost_kernel, dim3(rows), dim3(PH_THREADS), 0, s, p);
  HIP_CHECK(hipGetLastError());
}

}  // namespace ohw

using namespace ohw;

extern "C" {

int ohw_phrase_table_build_host(const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases, int eot, ohw_phrase_table* out) {
  return ph_guard([&] { phrase_table_build_host(tokens, offsets, boosts, n_phrases, eot, out); });
}

int ohw_phrase_boost_host(const ohw_phrase_table* table, const int32_t* history, int n_cur, float* row, int n_vocab) {
  return ph_guard([&] { phrase_boost_host(table, history, n_cur, row, n_vocab); });
}

}  // extern "C"
