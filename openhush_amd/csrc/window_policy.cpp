// window_policy.cpp — see window_policy.hpp.  Host only.
#include "window_policy.hpp"

#include <algorithm>

namespace ohw {

SeqEval evaluate_sequence(const ohw_special_tokens& tk, const int32_t* tok, const float* plog, int n, int seek, int seek_end, int n_max,
                          bool no_timestamps, int window_mode) {
  SeqEval r;
  bool has_ts = false;
  int stop = n;
  for (int i = 0; i < n; ++i) {
    const int t = tok[i];
    if (t > tk.timestamp_begin) {
      const int nd = 2 * (t - tk.timestamp_begin);
      if (has_ts && r.seek_delta > nd && r.result_len < i) { r.failed = true; stop = i + 1; break; }
      r.seek_delta = nd; r.result_len = i + 1; has_ts = true;
    }
    const bool audio_end = seek + r.seek_delta + 100 >= seek_end;
    if (t == tk.eot || (has_ts && audio_end)) {
      if (r.result_len == 0 && !no_timestamps) {
        if (audio_end) r.result_len = i + 1;
        else { r.failed = true; stop = i + 1; break; }
      }
      if (no_timestamps) { r.result_len = i + 1; r.seek_delta = 3000; }
      r.completed = true; stop = i + 1;
      break;
    }
    if (i == n_max - 1 && (r.result_len == 0 || r.seek_delta < 1500)) { r.failed = true; stop = i + 1; break; }
  }
  r.n_sampled = stop;
  if (r.result_len > 0) {
    double sum = 0.0;
    for (int i = 0; i < r.result_len; ++i) sum += plog[i];
    r.avg_logprob = (float)(sum / r.result_len);
    const int n32 = std::min(32, r.result_len), i0 = r.result_len - n32;
    double ent = 0.0;
    for (int i = i0; i < r.result_len; ++i) {
      bool first = true;
      int cnt = 0;
      for (int j = i0; j < r.result_len; ++j) if (tok[j] == tok[i]) { if (j < i) first = false; ++cnt; }
      if (first) { const double pr = (double)cnt / n32; ent -= pr * std::log(pr); }
    }
    r.entropy = (float)ent;
  }
  int keep = r.failed ? stop : (window_mode == OHW_WINDOW_SEEK ? r.result_len : stop);
  while (keep > 0 && tok[keep - 1] == tk.eot) --keep;
  r.n_keep = keep;
  return r;
}

bool needs_fallback(const SeqEval& r, const ohw_decode_policy& q, float no_speech_prob, bool is_last) {
  if (is_last) return false;
  const bool failed = r.failed || r.result_len == 0 || r.entropy < q.entropy_thold;
  return failed || (r.avg_logprob < q.logprob_thold && no_speech_prob < q.no_speech_thold);
}

bool is_no_speech(const WindowRun& r, const ohw_decode_policy& q) { return r.nosp > q.no_speech_thold && r.ev.avg_logprob < q.logprob_thold; }

std::vector<float> ladder(const ohw_decode_policy& q) {
  std::vector<float> t;
  if (q.temperature_inc > 0.0f)
    for (float x = q.temperature_inc; x < 1.0f + 1e-6f && t.size() < 16; x += q.temperature_inc) t.push_back(x);
  return t;
}

}  // namespace ohw

// ---- the test hook: the two rules above on plain arrays (include/ohw.h) ----------------------------------------------------
extern "C" {

int ohw_seq_eval_host(const ohw_special_tokens* tok, const int32_t* tokens, const float* plogs, int n, int seek, int seek_end, int n_max,
                      int no_timestamps, int window_mode, ohw_seq_eval* out) {
  if (!tok || !out || n < 0 || (n > 0 && (!tokens || !plogs))) return OHW_E_INVALID_ARG;
  const ohw::SeqEval r = ohw::evaluate_sequence(*tok, tokens, plogs, n, seek, seek_end, n_max, no_timestamps != 0, window_mode);
  *out = ohw_seq_eval{r.n_sampled, r.result_len, r.n_keep, r.seek_delta, r.failed ? 1 : 0, r.completed ? 1 : 0, r.avg_logprob, r.entropy};
  return OHW_OK;
}

int ohw_needs_fallback_host(const ohw_seq_eval* ev, const ohw_decode_policy* q, float no_speech_prob, int is_last) {
  if (!ev || !q) return OHW_E_INVALID_ARG;
  ohw::SeqEval r;
  r.n_sampled = ev->n_sampled; r.result_len = ev->result_len; r.n_keep = ev->n_keep; r.seek_delta = ev->seek_delta;
  r.failed = ev->failed != 0; r.completed = ev->completed != 0; r.avg_logprob = ev->avg_logprob; r.entropy = ev->entropy;
  return ohw::needs_fallback(r, *q, no_speech_prob, is_last != 0) ? 1 : 0;
}

int ohw_batch_windows_host(int max_batch, int beam_size, int best_of) {
  if (max_batch < 1 || (beam_size != 0 && (beam_size < 2 || beam_size > 5)) || best_of < 1 || best_of > 5) return OHW_E_INVALID_ARG;
  const int wb = max_batch / std::max(std::max(best_of, beam_size), 1);
  return wb < 1 ? OHW_E_INVALID_ARG : wb;
}

// best-of sampling: which of a rung's n judged candidates is kept (include/ohw.h).  The engine's rung calls
// this function itself
int ohw_best_of_pick_host(const ohw_seq_eval* ev, int n, const ohw_decode_policy* q, int* kept) {
  if (!ev || !q || !kept || n < 1 || n > 5) return OHW_E_INVALID_ARG;
  int best = -1;
  for (int j = 0; j < n; ++j) {
    if (ev[j].failed != 0 || ev[j].entropy < q->entropy_thold) continue;          // out
    if (best < 0 || ev[j].avg_logprob > ev[best].avg_logprob) best = j;           // strictly better only: the lowest j among equals
  }
  *kept = best < 0 ? 0 : best;
  return OHW_OK;
}

}  // extern "C"
