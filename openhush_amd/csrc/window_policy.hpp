// window_policy.hpp — whisper.cpp's per-window bookkeeping (whisper_full_with_state as recalled):
// the loop exits, the acceptance test, the no-speech rule, the temperature ladder.  Host only: no HIP include, no GPU call.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ohw.h"

namespace ohw {

struct SeqEval {
  int n_sampled = 0;     // tokens up to and including the one that ended the pass
  int result_len = 0;    // whisper.cpp result_len: up to and including the last timestamp token (> token_beg)
  int n_keep = 0;        // tokens that reach the text
  int seek_delta = 3000; // 10 ms frames the window advances by
  bool failed = false, completed = false;
  float avg_logprob = -INFINITY, entropy = 0.f;
};

// one decoded window: the pass that was kept
struct WindowRun {
  std::vector<int32_t> tok;   // sampled tokens of the kept pass (end-of-text last when sampled)
  std::vector<float> plog;
  float nosp = 0.f, temp = 0.f;
  SeqEval ev;
  bool pending = false, t0_failed = false;
  float list_lp = __builtin_nanf("");   // command lists: the pass's list_logprob (NaN: no list, or no step wrote one)
  std::vector<int32_t> al_idx;   // word timestamps: start index of every kept text token, then the end of the last (empty: not aligned)
  std::vector<ohw_token_score> sc;   // confidence: the score of every kept text token, then end-of-text's (empty: not scored)
};

// frames of 10 ms whisper.cpp attributes to n samples: mel.n_len_org = 1 + (n + 200 - 400) / 160
inline int mel_frames(int64_t n) { return (int)(1 + (n + 200 - 400) / 160); }

// One sampled sequence, judged after the fact (greedy decoding is causal: cutting at the first exit the walk finds equals
// having stopped there).  tok[0..n): the sampled tokens, the end-of-text token last when it was sampled.
//   exits      end-of-text; a timestamp that leaves less than 1 s of audio (seek + seek_delta + 100 >= seek_end);
//              failure when timestamps go back, when end-of-text arrives with no timestamp and audio left, or when the
//              loop reaches n_max without a timestamp past the middle of the window (the repetition-loop guard)
//   score      average log-probability and token-frequency entropy of the last 32 of the first result_len tokens
//   kept       fixed 30 s cuts: everything before the exit (each window is decoded once); seek loop: result_len tokens
//              (what follows the last timestamp is decoded again by the next window)
SeqEval evaluate_sequence(const ohw_special_tokens& tk, const int32_t* tok, const float* plog, int n, int seek, int seek_end, int n_max,
                          bool no_timestamps, int window_mode);

// does the pass go to the next temperature?  Never at the last one
bool needs_fallback(const SeqEval& r, const ohw_decode_policy& q, float no_speech_prob, bool is_last);

// whisper.cpp (>= 1.7.3 as recalled): a window whose no-speech probability is high AND whose text is unlikely is dropped
bool is_no_speech(const WindowRun& r, const ohw_decode_policy& q);
// tokens of the window that reach the text: none of a no-speech window
inline int kept_tokens(const WindowRun& r, const ohw_decode_policy& q) { return is_no_speech(r, q) ? 0 : r.ev.n_keep; }

// a SeqEval as the C ABI carries it (ohw_seq_eval_host, ohw_best_of_pick_host)
inline ohw_seq_eval seq_eval_c(const SeqEval& r) {
  return ohw_seq_eval{r.n_sampled, r.result_len, r.n_keep, r.seek_delta, r.failed ? 1 : 0, r.completed ? 1 : 0, r.avg_logprob, r.entropy};
}

// the temperatures after T = 0: temperature_inc, 2 * temperature_inc, ... up to 1.0
std::vector<float> ladder(const ohw_decode_policy& q);

}  // namespace ohw
