// transcribe.cpp — the engine's transcribe paths after validation: a window decoder (TranscribeCall: T = 0 pass, temperature
// ladder, alignment, text assembly; window_policy.hpp holds the rules) and four drivers over it - the seek loop and the fixed
// 30 s cuts of one recording (engine_transcribe), the short batch and the long-form batch (many recordings).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>

#include "host_engine.hpp"
#include "logit_rules.hpp"
#include "model.hpp"
#include "window_policy.hpp"

namespace ohw {
LogitRules& state_rules(ohw_state* st);
void state_share_recording(ohw_state* dst, ohw_state* src);
void state_drop_recording(ohw_state* st);
void state_set_graph_max_batch(ohw_state* st, int max_batch);
}
using namespace ohw;

namespace {
void check(int rc) { if (rc != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: " + g_last_error); }   // reference :266-268

// per-decode scratch: one per lane when several batches decode side by side
// one best-of rung of one window (ohw_engine_last_candidates): {window, T * 1000, N, kept}, then {n, tokens} per candidate; the
// candidates' log-probabilities beside it
struct CandRec { int32_t window; std::vector<int32_t> rec; std::vector<float> lps; };

struct Scratch {
  std::vector<CandRec> cands;
  std::vector<int32_t> toks, ntok, eot, trace;
  std::vector<float> lps, nsp, logits;
  std::vector<WindowRun> runs;
  Scratch(int B, int max_tok) : toks((size_t)B * max_tok), ntok((size_t)B), eot((size_t)B), lps((size_t)B * (max_tok + 1)), nsp((size_t)B) {}
  ohw_greedy_result greedy_result() {
    ohw_greedy_result gr{};
    gr.tokens = toks.data(); gr.n_tokens = ntok.data(); gr.token_logprobs = lps.data(); gr.ended_by_eot = eot.data(); gr.no_speech_prob = nsp.data();
    return gr;
  }
};

// whisper.cpp seeds decoder j's generator with j once per whisper_full call.  nr decoders' sets of N (best-of sampling: candidate
// j of entry i is v[i * N + j]); N = 1 is the one generator seeded with 0
struct Rngs {
  std::vector<ohw_rng*> v;
  explicit Rngs(size_t nr, int N = 1) { for (size_t i = 0; i < nr * (size_t)N; ++i) v.push_back(ohw_rng_new((uint32_t)(i % (size_t)N))); }
  ~Rngs() { for (ohw_rng* r : v) ohw_rng_free(r); }
};

// carried context (ohw_engine_set_carry_context; the seek loops only): one history per recording of the call, seeded with the
// initial prompt and moved on by ohw_carry_step_host after every window; `next` is what the recording's next window decodes
// behind at T = 0
struct Carry { std::vector<int32_t> hist, next; int n_hist = 0; };

// what varies from one decode batch to the next; B entries each
struct Batch {
  ohw_state* st = nullptr;
  int B = 0;
  const int* seek = nullptr;                               // first frame of every window in its recording, 10 ms frames
  const int* seek_end = nullptr;                           //   and the frame its recording ends at
  int64_t w0 = 0;                                          // window index of entry 0 in the trace
  const int32_t* langs = nullptr;                          // language ids read back from the state's table (null: the call's for all)
  const std::vector<int32_t>* const* ctx = nullptr;        // carried context per entry (null: the initial prompt for all)
  ohw_rng* const* rngs = nullptr;                          // the ladder's generators: best_of per entry, candidate j of entry b at [b * best_of + j]
};

// The window decoder of one transcribe call: constant for the call, so lane threads share it, each with its own Scratch and Batch
struct TranscribeCall {
  ohw_engine* const e;
  ohw_sample_params sp;
  const ohw_special_tokens& tk;
  const ohw_decode_policy pol;
  const int max_tok, V;
  int n_max = 0;
  std::vector<float> temps;            // the ladder's temperatures after T = 0
  // ohw_engine_set_beam_size: the T = 0 pass is a beam search of K rows per window, so a decode batch holds max_batch / K
  // windows (WB); beam calls run one batch after the other on the engine's own state
  // ohw_engine_set_best_of: every rung above T = 0 samples best_N rows per pending window on the device (rung_best_of), so a
  // batch holds max_batch / max(best_N, beam_K, 1) windows, and the call runs like a beam call
  int beam_K = 0, WB = 1, best_N = 1;
  int32_t prompt[8];                   // the task prompt: sot [, language, task] [, no_timestamps]
  int n_prompt = 0;
  const bool carrying;
  // detect_samples: the recording whose first window is detected when the engine detects (null: a batch path, it detects per recording)
  TranscribeCall(ohw_engine* e_, const float* detect_samples, int64_t detect_n)
      : e(e_), tk(e_->ctx->tok), pol(e_->policy), max_tok(e_->ctx->hp.n_text_ctx), V(e_->ctx->hp.n_vocab),
        carrying(e_->carry_max != 0 && e_->window_mode == OHW_WINDOW_SEEK) {
    ohw_default_sample_params(e->ctx, &sp);
    // reference :246-248: "auto" skips set_language and whisper.cpp keeps its default "en"
    sp.lang_id = e->language == "auto" ? 0 : ohw_lang_code_to_id(e->language.c_str());
    // reference :251-257 passes !translate to whisper-rs on the claim that the binding is inverted;
    // the resulting behaviour the reference documents is: config translate=true -> translate task
    sp.translate = e->translate ? 1 : 0;
    if (e->force_len > 0) { sp.force_len = std::min(e->force_len, sp.n_max); sp.n_max = sp.force_len; }      // bench: fixed decode length
    if (sp.lang_id >= tk.n_langs) throw Error(OHW_E_TRANSCRIBE, "language is not supported by this model");
    // ohw_engine_set_detect_language: one detection per call, on the first window (or the id the pool detected); every window
    // of every schedule then runs at that id, exactly as an engine created with its code
    e->last_lang_id = sp.lang_id;
    e->last_lang_prob = 1.f;
    if (detect_samples && engine_detects(e)) {
      if (e->given_lang >= 0) { e->last_lang_id = e->given_lang; e->last_lang_prob = e->given_prob; }
      else e->last_lang_id = engine_detect_first_window(e, detect_samples, detect_n, &e->last_lang_prob);
      sp.lang_id = e->last_lang_id;
    }
    e->last.clear();
    e->last_trace.clear();
    n_max = sp.n_max;
    temps = ladder(pol);
    beam_K = e->beam_size;
    best_N = temps.empty() ? 1 : e->best_of;       // no rung above T = 0: nothing of best-of applies, batch size included
    WB = ohw_batch_windows_host(e->max_batch, beam_K, best_N);
    if (WB < 1) throw Error(OHW_E_INVALID_ARG, "transcribe: beam size or best_of exceeds max_batch");
    e->last_cands.clear();
    e->last_cand_lps.clear();
    e->last_seams.clear();
    e->last_win_tokens.clear();
    e->last_win_offsets.clear();
    prompt[n_prompt++] = tk.sot;
    if (V >= 51865) { prompt[n_prompt++] = tk.sot + 1 + sp.lang_id; prompt[n_prompt++] = sp.translate ? tk.translate : tk.transcribe; }
    if (sp.no_timestamps) prompt[n_prompt++] = tk.no_timestamps;
  }
  static void trace(Scratch& sc, int64_t window, float temp, const std::vector<int32_t>& t) {
    sc.trace.push_back((int32_t)window); sc.trace.push_back((int32_t)std::lround(temp * 1000.f)); sc.trace.push_back((int32_t)t.size());
    sc.trace.insert(sc.trace.end(), t.begin(), t.end());
  }
  SeqEval evaluate(const WindowRun& r, const Batch& bt, int b) const {
    return evaluate_sequence(tk, r.tok.data(), r.plog.data(), (int)r.tok.size(), bt.seek[b], bt.seek_end[b], n_max, sp.no_timestamps != 0, e->window_mode);
  }
  // the kept pass of a window moves its recording's history on
  void carry_step(Carry& c, const WindowRun* r) const {
    std::vector<int32_t> out((size_t)std::max(1, max_tok / 2));
    int n_out = 0;
    const int rc = ohw_carry_step_host(c.hist.data(), &c.n_hist, max_tok, r ? r->tok.data() : nullptr, r ? kept_tokens(*r, pol) : 0, r ? r->temp : 0.f,
                                       e->carry_max, out.data(), &n_out);
    if (rc != OHW_OK) throw Error(rc, "carry_context: " + g_last_error);
    c.next.assign(out.begin(), out.begin() + n_out);
  }
  void carry_init(Carry& c) const {
    c.hist.assign((size_t)std::max(1, max_tok / 2), 0);
    c.n_hist = (int)std::min(e->prompt.size(), c.hist.size());
    std::copy(e->prompt.end() - c.n_hist, e->prompt.end(), c.hist.begin());
    carry_step(c, nullptr);
  }
  // the context of every window of the batch: the carried one, else the initial prompt (ohw_engine_set_initial_prompt); with
  // none set and none ever set, nothing is called.  The ladder clears the table before its first pass with T >= 0.5
  // (whisper.cpp's rule, as recalled), so every batch sets it again here
  void apply_prompt(const Batch& bt) const {
    const int B = bt.B;
    // a slot whose history is empty gets count 0; a round in which every history is empty runs with no table at all
    size_t np = bt.ctx ? 0 : e->prompt.size();
    for (int b = 0; bt.ctx && b < B; ++b) np = std::max(np, bt.ctx[b]->size());
    if (np == 0) {
      if (e->prompt_used) check(ohw_state_set_window_prompt(bt.st, nullptr, 0, nullptr, 0));
      return;
    }
    std::vector<int32_t> tab((size_t)B * np, 0), cnt((size_t)B, 0);
    for (int b = 0; b < B; ++b) {
      const std::vector<int32_t>& c = bt.ctx ? *bt.ctx[b] : e->prompt;
      cnt[(size_t)b] = (int32_t)c.size();
      std::copy(c.begin(), c.end(), tab.begin() + (long)((size_t)b * np));
    }
    if (bt.ctx) e->prompt_used = true;
    check(ohw_state_set_window_prompt(bt.st, tab.data(), (int)np, cnt.data(), B));
  }
  // row b of a greedy, beam or sample result as a WindowRun: tokens (end-of-text last when it ended the row), log-probabilities,
  // no-speech probability, and the row's evaluation.  cut: the row was not decoded under whisper.cpp's loop exits (beam search is
  // not causal, the device sampler runs to the end), so it is cut at the first exit and judged again; a greedy row stays whole
  // row: the result row of entry b when it is not b itself (best-of sampling: one of the entry's candidates)
  void unpack(const Scratch& sc, const Batch& bt, int b, bool cut, WindowRun& r, int row = -1) const {
    const int eb = b;
    if (row >= 0) b = row;
    const int nt = sc.ntok[(size_t)b] + (sc.eot[(size_t)b] ? 1 : 0);
    r.tok.assign(&sc.toks[(size_t)b * max_tok], &sc.toks[(size_t)b * max_tok] + sc.ntok[(size_t)b]);
    if (sc.eot[(size_t)b]) r.tok.push_back(tk.eot);
    r.plog.assign(&sc.lps[(size_t)b * (max_tok + 1)], &sc.lps[(size_t)b * (max_tok + 1)] + nt);
    r.nosp = sc.nsp[(size_t)b];
    r.ev = evaluate(r, bt, eb);
    if (!cut) return;
    r.tok.resize((size_t)r.ev.n_sampled);
    r.plog.resize((size_t)r.ev.n_sampled);
    r.ev = evaluate(r, bt, eb);
  }
  // command lists: list_logprob of the device pass that just ran on the batch's state, into the runs of its active windows (every
  // device pass writes entry b for window b); nothing with no list set
  void read_list_logprob(const Batch& bt, const int32_t* active, std::vector<WindowRun>& runs) const {
    if (!state_rules(bt.st).cm.on) return;
    std::vector<float> lp((size_t)bt.B);
    check(ohw_state_command_list_logprob(bt.st, bt.B, lp.data()));
    for (int b = 0; b < bt.B; ++b)
      if (!active || active[b]) runs[(size_t)b].list_lp = lp[(size_t)b];
  }
  // T = 0: the device-resident greedy loop for B windows, or under ohw_engine_set_beam_size ohw_beam_search_ex in its place; then
  // whisper.cpp's bookkeeping per window.  A beam winner (with end-of-text when it came from the finished pool) has whisper.cpp's
  // loop exits applied after the search (a definition), not to every decoder during it; from there on it is
  // the greedy pass: needs_fallback, t0_failed, the no-speech rule, n_keep, segments, alignment.
  // The ladder that may follow is unchanged and safe after a search: it decodes rows 0 .. B-1 from position 0 (prefill,
  // prompt, steps), reads a row's self K/V only below the position it has itself written in that pass, without a kv_slot
  // table, and reads cross K/V by WINDOW index, which the search never moves - nothing it relies on is left in beam layout
  // (row w * K); its entries re-initialise n_past, the token history and the done flags themselves
  void pass_t0(Scratch& sc, const Batch& bt) const {
    apply_prompt(bt);
    if (beam_K > 0) {
      ohw_beam_result_ex br{};
      br.tokens = sc.toks.data(); br.n_tokens = sc.ntok.data(); br.token_logprobs = sc.lps.data(); br.ended_by_eot = sc.eot.data();
      br.no_speech_prob = sc.nsp.data();
      check(ohw_beam_search_ex(bt.st, &sp, bt.B, beam_K, max_tok, &br));
    } else {
      ohw_greedy_result gr = sc.greedy_result();
      check(ohw_greedy_ex(bt.st, &sp, bt.B, max_tok, &gr));
    }
    sc.runs.assign((size_t)bt.B, WindowRun());
    for (int b = 0; b < bt.B; ++b) {
      WindowRun& r = sc.runs[(size_t)b];
      unpack(sc, bt, b, beam_K > 0, r);
      r.t0_failed = needs_fallback(r.ev, pol, r.nosp, false);
      r.pending = needs_fallback(r.ev, pol, r.nosp, temps.empty());
      trace(sc, bt.w0 + b, 0.f, r.tok);
    }
    read_list_logprob(bt, nullptr, sc.runs);
  }
  // one rung sampled on the device (ohw_sample_pass: the greedy loop's replayed {step, sampler} with the temperature sampler)
  // from the host generators' pre-drawn doubles; the host then cuts each pass at whisper.cpp's loop exits and advances each
  // generator by the draws it kept, where the host rung would leave it
  void rung_device(Scratch& sc, const Batch& bt, const std::vector<int32_t>& active, float T, std::vector<WindowRun>& pass) const {
    std::vector<double> u((size_t)bt.B * max_tok, 0.0);
    const int n_draw = std::min(n_max, max_tok);
    for (int b = 0; b < bt.B; ++b)
      if (active[(size_t)b] && ohw_rng_uniforms(bt.rngs[b], n_draw, &u[(size_t)b * max_tok]) != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: generator");
    ohw_greedy_result gr = sc.greedy_result();
    check(ohw_sample_pass(bt.st, &sp, bt.B, max_tok, T, active.data(), u.data(), &gr));
    for (int b = 0; b < bt.B; ++b) {
      if (!active[(size_t)b]) continue;
      unpack(sc, bt, b, true, pass[(size_t)b]);
      if (ohw_rng_discard_draws(bt.rngs[b], pass[(size_t)b].ev.n_sampled) != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: generator");
    }
    read_list_logprob(bt, active.data(), pass);
  }
  // one rung of best-of sampling (ohw_engine_set_best_of): best_N candidates per pending window in ONE
  // ohw_sample_pass_n - candidate j draws from the entry's generator j, is cut and judged like rung_device's one row, and moves
  // its own generator on by the draws its cut pass used; ohw_best_of_pick_host keeps one, which is the rung's pass from here on
  void rung_best_of(Scratch& sc, const Batch& bt, const std::vector<int32_t>& active, float T, std::vector<WindowRun>& pass) const {
    const int N = best_N, R = bt.B * N;
    Scratch cs(R, max_tok);
    std::vector<double> u((size_t)R * max_tok, 0.0);
    const int n_draw = std::min(n_max, max_tok);
    for (int r = 0; r < R; ++r)
      if (active[(size_t)(r / N)] && ohw_rng_uniforms(bt.rngs[r], n_draw, &u[(size_t)r * max_tok]) != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: generator");
    ohw_greedy_result gr = cs.greedy_result();
    check(ohw_sample_pass_n(bt.st, &sp, bt.B, N, max_tok, T, active.data(), u.data(), &gr));
    for (int b = 0; b < bt.B; ++b) {
      if (!active[(size_t)b]) continue;
      std::vector<WindowRun> c((size_t)N);
      ohw_seq_eval ev[5];
      for (int j = 0; j < N; ++j) {
        unpack(cs, bt, b, true, c[(size_t)j], b * N + j);
        if (ohw_rng_discard_draws(bt.rngs[b * N + j], c[(size_t)j].ev.n_sampled) != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: generator");
        ev[j] = seq_eval_c(c[(size_t)j].ev);
      }
      int kept = 0;
      if (ohw_best_of_pick_host(ev, N, &pol, &kept) != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: best-of pick");
      CandRec cr;
      cr.window = (int32_t)(bt.w0 + b);
      cr.rec = {cr.window, (int32_t)std::lround(T * 1000.f), N, kept};
      for (const WindowRun& r : c) {
        cr.rec.push_back((int32_t)r.tok.size());
        cr.rec.insert(cr.rec.end(), r.tok.begin(), r.tok.end());
        cr.lps.insert(cr.lps.end(), r.plog.begin(), r.plog.end());
      }
      sc.cands.push_back(std::move(cr));
      pass[(size_t)b] = std::move(c[(size_t)kept]);
    }
    read_list_logprob(bt, active.data(), pass);      // the window's first candidate's: the candidates part ways behind the first token
  }
  // one rung sampled on the host: the device runs the decoder steps of the pending windows only and their logits cross PCIe
  // every step; a window stops inside the loop, at whisper.cpp's exits
  void rung_host(Scratch& sc, const Batch& bt, const std::vector<int32_t>& active, float T, std::vector<WindowRun>& pass) const {
    const int B = bt.B;
    std::vector<float>& logits = sc.logits;
    logits.resize((size_t)B * V);
    std::vector<int32_t> ptoks((size_t)B * n_prompt), past((size_t)B, 0), feed((size_t)B, tk.eot), npast((size_t)B, n_prompt), live = active;
    for (int b = 0; b < B; ++b) {
      std::memcpy(&ptoks[(size_t)b * n_prompt], prompt, (size_t)n_prompt * 4);
      if (bt.langs && V >= 51865) ptoks[(size_t)b * n_prompt + 1] = tk.sot + 1 + bt.langs[b];   // the table's ids, read back once per batch
    }
    // under a context table: the prefill for the pending windows, then the prompt at the context's length
    check(ohw_state_prefill(bt.st, B, active.data()));
    for (int b = 0; b < B; ++b) {
      past[(size_t)b] = std::max(0, ohw_state_window_prompt_len(bt.st, b));
      npast[(size_t)b] += past[(size_t)b];
    }
    check(ohw_decode_active(bt.st, ptoks.data(), n_prompt, past.data(), B, active.data(), logits.data()));
    for (int i = 0; i < n_max; ++i) {
      bool any_live = false;
      for (int b = 0; b < B; ++b) {
        if (!live[(size_t)b]) continue;
        WindowRun& r = pass[(size_t)b];
        float lp = 0.f;
        // the state's rules and its bias, in the device's order (LogitRules::apply and the samplers)
        check(state_rules(bt.st).apply_host(r.tok.data(), (int)r.tok.size(), &logits[(size_t)b * V], V, tk.eot, &r.list_lp));
        const int32_t t = ohw_sample_host(e->ctx, &sp, &logits[(size_t)b * V], r.tok.data(), (int)r.tok.size(), T, bt.rngs[b], &lp, &r.nosp);
        if (t < 0) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: host sampler");
        r.tok.push_back(t); r.plog.push_back(lp);
        const SeqEval ev = evaluate(r, bt, b);
        if (t == tk.eot || ev.completed || ev.failed || (int)r.tok.size() >= n_max || npast[(size_t)b] + 1 >= max_tok) live[(size_t)b] = 0;
        else { feed[(size_t)b] = t; any_live = true; }
      }
      if (!any_live) break;
      check(ohw_decode_active(bt.st, feed.data(), 1, npast.data(), B, live.data(), logits.data()));
      for (int b = 0; b < B; ++b) if (live[(size_t)b]) ++npast[(size_t)b];
    }
  }
  // the temperature ladder for the windows of a batch whose pass failed the acceptance test, drawn from std::mt19937 through
  // std::discrete_distribution as whisper.cpp's decoders do, on the pending windows' resident cross K/V; sampled by the host,
  // or by the device under ohw_engine_set_fallback_device - the same passes, generators and decisions
  void run_ladder(Scratch& sc, const Batch& bt) const {
    std::vector<WindowRun>& runs = sc.runs;
    for (size_t ti = 0; ti < temps.size(); ++ti) {
      std::vector<int32_t> active((size_t)bt.B, 0);
      bool any = false;
      for (int b = 0; b < bt.B; ++b) if (runs[(size_t)b].pending) { active[(size_t)b] = 1; any = true; }
      if (!any) break;
      const float T = temps[ti];
      std::vector<WindowRun> pass((size_t)bt.B);
      // passes with T < 0.5 decode behind the context; from the first pass with T >= 0.5 on the table is gone
      if (T >= 0.5f && (carrying || !e->prompt.empty())) check(ohw_state_set_window_prompt(bt.st, nullptr, 0, nullptr, 0));
      if (best_N > 1) rung_best_of(sc, bt, active, T, pass);
      else if (e->fallback_device) rung_device(sc, bt, active, T, pass);
      else rung_host(sc, bt, active, T, pass);
      for (int b = 0; b < bt.B; ++b) {
        if (!active[(size_t)b]) continue;
        WindowRun& r = pass[(size_t)b];
        r.temp = T;
        r.ev = evaluate(r, bt, b);
        r.t0_failed = runs[(size_t)b].t0_failed;
        r.pending = needs_fallback(r.ev, pol, r.nosp, ti + 1 == temps.size());
        trace(sc, bt.w0 + b, T, r.tok);
        runs[(size_t)b] = std::move(r);
      }
    }
  }
  // word timestamps: the kept pass of every window of a batch is aligned on the state that decoded it, while its cross K/V
  // is resident (before that state's next encode); windows with no kept text token are skipped.  frames: 10 ms frames of audio
  // confidence (ohw_engine_set_confidence): the same tokens are scored by the unconstrained model, in the alignment's own
  // replay when both are on (ohw_state_score with a start index output), alone when word timestamps are off
  void align_runs(Scratch& sc, ohw_state* st, int B, const int* frames) const {
    const bool al = !e->wt_heads.empty(), conf = e->confidence;
    if (!al && !conf) return;
    const int half = max_tok / 2;
    std::vector<int32_t> atok((size_t)B * half, 0), nt((size_t)B, 0), nf((size_t)B, 0), out((size_t)B * (half + 1), 0);
    bool any = false;
    for (int b = 0; b < B; ++b) {
      WindowRun& r = sc.runs[(size_t)b];
      r.al_idx.clear();
      r.sc.clear();
      const int keep = kept_tokens(r, pol);
      int k = 0;
      for (int i = 0; i < keep && k < half; ++i)
        if (r.tok[(size_t)i] < tk.eot) atok[(size_t)b * half + k++] = r.tok[(size_t)i];
      nt[(size_t)b] = k;
      nf[(size_t)b] = std::max(0, frames[b]);
      any = any || k > 0;
    }
    if (!any) return;
    if (al) check(ohw_state_set_align_heads(st, e->wt_heads.data(), (int)e->wt_heads.size()));
    std::vector<ohw_token_score> scores((size_t)(conf ? B * (half + 1) : 0));
    if (conf) check(ohw_state_score(st, &sp, atok.data(), half, nt.data(), B, scores.data(), al ? nf.data() : nullptr, al ? out.data() : nullptr));
    else check(ohw_state_align(st, &sp, atok.data(), half, nt.data(), nf.data(), B, out.data()));
    for (int b = 0; b < B; ++b) {
      if (nt[(size_t)b] == 0) continue;
      if (al) sc.runs[(size_t)b].al_idx.assign(&out[(size_t)b * (half + 1)], &out[(size_t)b * (half + 1)] + nt[(size_t)b] + 1);
      if (conf) sc.runs[(size_t)b].sc.assign(&scores[(size_t)b * (half + 1)], &scores[(size_t)b * (half + 1)] + nt[(size_t)b] + 1);
    }
  }
  // the decode of one batch of fixed cuts (each its own `full` call in whisper.cpp terms: seek 0, its own frame count as the end
  // of the audio, fresh generators) on whatever stream the state is set to; fills sc.runs and sc.trace; re-entrant per Scratch.
  // nsb: samples per window; langs: as Batch::langs
  void decode_windows(Scratch& sc, ohw_state* st, int64_t w0, int B, const int32_t* nsb, const int32_t* langs = nullptr) const {
    std::vector<int> zero((size_t)B, 0), ends((size_t)B);
    for (int b = 0; b < B; ++b) ends[(size_t)b] = mel_frames(nsb[b]);
    Batch bt{st, B, zero.data(), ends.data(), w0, langs, nullptr, nullptr};
    pass_t0(sc, bt);
    // like a call with less than 1 s of audio, a cut of at most 100 frames yields nothing; its trace record remains
    for (int b = 0; b < B; ++b) if (ends[(size_t)b] <= 100) { sc.runs[(size_t)b] = WindowRun(); sc.runs[(size_t)b].ev.result_len = 0; }
    bool any = false;
    for (int b = 0; b < B; ++b) any = any || sc.runs[(size_t)b].pending;
    if (any) {
      Rngs lr((size_t)B, best_N);
      bt.rngs = lr.v.data();
      run_ladder(sc, bt);
    }
    align_runs(sc, st, B, ends.data());
  }
  // one window's kept pass onto the end of a transcript.  t_off: the window's offset in the recording, t_end: the earlier of the
  // window's end and the recording's end (seconds); ctx: what the window's T = 0 pass was decoded behind
  // cut (stitched windows): the kept-token range [first, end) that reaches the transcript and the seam times of its two sides;
  // null: the whole window
  struct Cut { int first, end; float t_left, t_right; };
  void emit(const WindowRun& r, double t_off, double t_end, Transcript& out, const std::vector<int32_t>& ctx, const Cut* cut = nullptr) const {
    std::string& text = out.text;
    const bool no_speech = is_no_speech(r, pol);
    const int keep = kept_tokens(r, pol);
    const int first = cut ? std::min(std::max(cut->first, 0), keep) : 0, end = cut ? std::min(std::max(cut->end, first), keep) : keep;
    size_t k0 = 0, nt_all = 0;                                         // text tokens in front of the range, and of the whole window
    for (int i = 0; i < keep; ++i)
      if (r.tok[(size_t)i] < tk.eot) { ++nt_all; if (i < first) ++k0; }
    const size_t win_text0 = text.size(), tt0 = out.token_times.size(), wd0 = out.words.size(), sg0 = out.segments.size();
    const size_t tp0 = out.token_probs.size(), wp0 = out.word_probs.size();
    std::vector<size_t> byte_off((size_t)keep + 1, text.size());       // text offset in front of every kept token
    std::vector<int32_t> tlen;                                         // byte length of every kept TEXT token
    std::vector<int> tpos;                                             //   and its position among the kept tokens
    for (int i = first; i < end; ++i) {
      byte_off[(size_t)i] = text.size();
      out.tokens.push_back(r.tok[(size_t)i]);
      if (r.tok[(size_t)i] < tk.eot) {                                    // segment text = text tokens only (:271-279)
        const char* sp_ = nullptr;
        const int len = ohw_token_text(e->ctx, r.tok[(size_t)i], &sp_);
        text.append(sp_, (size_t)len);
        tlen.push_back(len); tpos.push_back(i);
      }
    }
    for (int i = end; i <= keep; ++i) byte_off[(size_t)i] = text.size();
    if (keep > 0) {
      // segments (always): the text between consecutive timestamp tokens
      std::vector<ohw_token_span> spans((size_t)keep);
      const int ns_ = ohw_segments_host(r.tok.data(), keep, &tk, (float)t_off, (float)t_end, spans.data(), keep);
      for (int s = 0; s < ns_; ++s) {
        ohw_token_span sp_ = spans[(size_t)s];
        if (cut && ohw_stitch_clip_segment_host(&spans[(size_t)s], first, end, cut->t_left, cut->t_right, &sp_) != 1) continue;
        const size_t o0 = byte_off[(size_t)sp_.first], o1 = byte_off[(size_t)sp_.end];
        out.segments.push_back(ohw_span_time{o0, o1 - o0, sp_.t0, sp_.t1});
      }
    }
    if (!r.al_idx.empty() && r.al_idx.size() == nt_all + 1) {
      // token times, and words by the host rule (include/ohw.h)
      const int32_t window = (int32_t)out.quality.size();
      const size_t first_tt = out.token_times.size();
      for (size_t k = 0; k < tlen.size(); ++k)
        out.token_times.push_back(ohw_token_time{r.tok[(size_t)tpos[k]], window, (float)t_off + (float)r.al_idx[k0 + k] * 0.02f,
                                                 (float)t_off + (float)r.al_idx[k0 + k + 1] * 0.02f});
      std::vector<int32_t> starts(tlen.size(), 0);
      (void)ohw_word_starts_host(text.data() + win_text0, tlen.data(), (int)tlen.size(), starts.data());
      for (size_t k = 0; k < tlen.size(); ++k) {
        const ohw_token_time& tt = out.token_times[first_tt + k];
        const size_t o0 = byte_off[(size_t)tpos[k]];
        if (starts[k] || out.words.size() == wd0) out.words.push_back(ohw_span_time{o0, 0, tt.t0, tt.t1});
        ohw_span_time& w = out.words.back();
        w.text_len = o0 + (size_t)tlen[k] - w.text_off;
        w.t1 = tt.t1;
      }
    }
    if (e->confidence) {
      // token probabilities, word probabilities by the host rules (include/ohw.h), one info entry per segment of the window
      const bool scored = !r.sc.empty() && r.sc.size() == nt_all + 1;
      std::vector<float> lpt(scored ? tlen.size() : 0);
      if (scored) {
        const int32_t window = (int32_t)out.quality.size();
        for (size_t k = 0; k < tlen.size(); ++k) {
          ohw_token_prob tp{r.tok[(size_t)tpos[k]], window, 0.f, 0.f, r.plog[(size_t)tpos[k]], r.sc[k0 + k].top_id, 0.f};
          (void)ohw_token_prob_host(&r.sc[k0 + k], &tp.logprob_text, &tp.logprob_all, &tp.top_logprob_text);
          lpt[k] = tp.logprob_text;
          out.token_probs.push_back(tp);
        }
        std::vector<int32_t> starts(tlen.size(), 0);
        std::vector<float> wp(tlen.size(), 0.f);
        (void)ohw_word_starts_host(text.data() + win_text0, tlen.data(), (int)tlen.size(), starts.data());
        const int n_wp = ohw_word_probs_host(lpt.data(), starts.data(), (int)tlen.size(), wp.data());
        for (size_t k = 0; k < tlen.size(); ++k) {
          const size_t o0 = byte_off[(size_t)tpos[k]];
          if (starts[k] || out.word_probs.size() == wp0) out.word_probs.push_back(ohw_word_prob{o0, 0, 0.f});
          ohw_word_prob& w = out.word_probs.back();
          w.text_len = o0 + (size_t)tlen[k] - w.text_off;
        }
        for (size_t i = 0; i < out.word_probs.size() - wp0 && (int)i < n_wp; ++i) out.word_probs[wp0 + i].probability = wp[i];
      }
      for (size_t s = sg0; s < out.segments.size(); ++s) {
        // the segment's text tokens: those whose bytes lie inside its span (a segment is a run of kept tokens)
        double sum = 0.0;
        int cnt = 0;
        for (size_t k = 0; scored && k < tlen.size(); ++k) {
          const size_t o = byte_off[(size_t)tpos[k]];
          if (o >= out.segments[s].text_off && o + (size_t)tlen[k] <= out.segments[s].text_off + out.segments[s].text_len) { sum += lpt[k]; ++cnt; }
        }
        out.segment_info.push_back(ohw_segment_info{cnt > 0 ? (float)(sum / cnt) : __builtin_nanf(""), r.nosp, r.temp});
      }
    }
    out.marks.push_back(WindowMark{win_text0, (int32_t)(out.token_times.size() - tt0), (int32_t)(out.words.size() - wd0), (int32_t)(out.segments.size() - sg0),
                                   (int32_t)(out.token_probs.size() - tp0), (int32_t)(out.word_probs.size() - wp0)});
    out.contexts.push_back(ctx);
    if (const LogitRules& rules = state_rules(e->state); rules.cm.on) {
      const int id = ohw_command_match_host(&rules.cm.host, r.tok.data(), keep);
      const int32_t phrase = id < 0 ? -1 : (size_t)id < e->cmd_index.size() ? e->cmd_index[(size_t)id] : id;
      out.commands.push_back(ohw_command_hit{(int32_t)out.quality.size(), phrase, r.list_lp});
    }
    ohw_window_quality q{};
    q.n_tokens = keep; q.avg_logprob = r.ev.avg_logprob; q.entropy = r.ev.entropy; q.would_fallback = r.t0_failed ? 1 : 0;
    q.temperature = r.temp; q.no_speech_prob = r.nosp; q.no_speech = no_speech ? 1 : 0; q.seek_delta = r.ev.seek_delta;
    q.result_len = r.ev.result_len; q.failed = r.ev.failed ? 1 : 0;
    out.quality.push_back(q);
  }
  // a batch records its passes in the order it ran them (every window's T = 0 pass, then the ladder's rungs); the trace lists
  // them window by window, each window's passes in order, so it reads the same however the windows were batched
  void flush_trace(Scratch& sc) const {
    std::vector<std::pair<int32_t, size_t>> recs;            // (window, offset of the record)
    for (size_t i = 0; i + 3 <= sc.trace.size(); i += 3 + (size_t)sc.trace[i + 2]) recs.emplace_back(sc.trace[i], i);
    std::stable_sort(recs.begin(), recs.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    for (const auto& r : recs) e->last_trace.insert(e->last_trace.end(), sc.trace.begin() + (long)r.second, sc.trace.begin() + (long)(r.second + 3 + (size_t)sc.trace[r.second + 2]));
    sc.trace.clear();
    // the best-of rungs alike: window by window, a window's rungs in the order they ran
    std::stable_sort(sc.cands.begin(), sc.cands.end(), [](const CandRec& a, const CandRec& b) { return a.window < b.window; });
    for (const CandRec& c : sc.cands) {
      e->last_cands.insert(e->last_cands.end(), c.rec.begin(), c.rec.end());
      e->last_cand_lps.insert(e->last_cand_lps.end(), c.lps.begin(), c.lps.end());
    }
    sc.cands.clear();
  }
};

// the call's audio context on every state it may run on
void apply_ctx(ohw_engine* e, int call_ctx) {
  each_state(e, [&](ohw_state* st) { check(ohw_state_set_audio_ctx(st, call_ctx)); });
}
// a fixed context never drops audio silently: a window that holds samples past it fails the call
void check_window_fits(int call_ctx, int64_t window, int64_t win_samples) {
  if (call_ctx > 0 && win_samples > (int64_t)call_ctx * 320)
    throw Error(OHW_E_INVALID_ARG, "audio_ctx " + std::to_string(call_ctx) + " covers " + std::to_string((int64_t)call_ctx * 320) + " samples, window " +
                                       std::to_string(window) + " holds " + std::to_string(win_samples));
}

// a language per entry of a batch on the state's table; OHW_LANG_DETECT entries are detected.  The table is read back once, when
// something was detected or always.  Returns whether something was detected
bool apply_window_langs(ohw_state* st, std::vector<int32_t>& langs, bool always_read_back) {
  const int B = (int)langs.size();
  const bool any_detect = std::find(langs.begin(), langs.end(), OHW_LANG_DETECT) != langs.end();
  check(ohw_state_set_window_lang(st, langs.data(), B));
  if (any_detect) check(ohw_state_detect_window_lang(st, B));
  if (any_detect || always_read_back) check(ohw_state_window_lang(st, B, langs.data(), nullptr));
  return any_detect;
}

// ---- whisper.cpp's seek loop as recalled: sequential windows, advanced by the last timestamp; one generator
// for the whole call ----
void transcribe_seek(const TranscribeCall& tc, const float* samples, int64_t n) {
  ohw_engine* e = tc.e;
  Rngs rngs(1, tc.best_N);
  Scratch sc(1, tc.max_tok);
  Carry carry;
  if (tc.carrying) tc.carry_init(carry);
  const std::vector<int32_t>* ctx = &carry.next;
  const int seek_end = mel_frames(n), call_ctx = engine_call_ctx(e, n);
  int seek = 0;
  int64_t w = 0;
  // whisper.cpp computes the log-mel spectrogram of the whole input once (the clamp uses its global maximum) and every
  // window reads 3000 frames of it at its seek offset
  if (seek_end >= 100) check(ohw_recording_set(e->state, samples, n, 0, nullptr));
  apply_ctx(e, call_ctx);
  while (seek_end >= 100 && seek + 100 < seek_end) {
    const int32_t seek32 = seek;
    check_window_fits(call_ctx, w, std::min<int64_t>(CHUNK_SAMPLES, n - (int64_t)seek * HOP));
    check(ohw_mel_seek(e->state, &seek32, 1, nullptr));      // 3000 frames of the recording-wide spectrogram
    check(ohw_encode(e->state, 1));
    const Batch bt{e->state, 1, &seek, &seek_end, w, nullptr, tc.carrying ? &ctx : nullptr, rngs.v.data()};
    tc.pass_t0(sc, bt);
    tc.run_ladder(sc, bt);
    const int win_frames = std::min(CHUNK_FRAMES, seek_end - seek);
    tc.align_runs(sc, e->state, 1, &win_frames);
    tc.flush_trace(sc);
    const WindowRun& r = sc.runs[0];
    tc.emit(r, seek * 0.01, std::min(seek * 0.01 + 30.0, (double)n / 16000.0), e->last, tc.carrying ? carry.next : e->prompt);
    if (tc.carrying) tc.carry_step(carry, &r);
    seek += r.ev.seek_delta > 0 ? r.ev.seek_delta : 3000;
    ++w;
  }
  if (tc.carrying && w > 0) check(ohw_state_set_window_prompt(e->state, nullptr, 0, nullptr, 0));
}

// ---- host-side windowing: fixed 30 s cuts (BASELINE.json north_star).  The pool deals the recording's windows
// round-robin: this engine takes windows win_first, win_first + win_step, ... of the WHOLE recording it is handed (no copy, and -
// FIXED_RECORDING_MEL - the real neighbouring samples and the recording-wide clamp maximum); k counts this engine's windows,
// rec_win(k) is the window of the recording ----
struct FixedCuts {
  const TranscribeCall& tc;
  ohw_engine* const e;
  const float* const samples;
  const int64_t n, win_first, win_step;
  // stitched windows (ohw_engine_set_stitch; an engine that takes the whole recording): neighbouring windows start `hop` samples
  // apart and share the rest, every window's kept pass waits in `held` until finish() has cut them at the seams.  Off: the hop
  // is the window, and nothing below differs from cuts every 30 s
  const bool stitch;
  const int64_t hop, n_win, n_batches;
  const int WB;
  const bool rec_mel;        // cut from the spectrogram of the whole recording, which e->state holds, instead of each cut on its own
  mutable std::vector<WindowRun> held;
  mutable std::map<ohw_state*, std::vector<float>> staged;      // front ends are enqueued by the calling thread only
  FixedCuts(const TranscribeCall& tc_, const float* samples_, int64_t n_, int64_t first, int64_t step)
      : tc(tc_), e(tc_.e), samples(samples_), n(n_), win_first(first), win_step(step), stitch(tc_.e->stitch_ms > 0 && step == 1),
        hop(stitch ? CHUNK_SAMPLES - (int64_t)tc_.e->stitch_ms * 16 : CHUNK_SAMPLES),
        n_win(share_of(n_, first, step, hop)), n_batches((n_win + tc_.WB - 1) / tc_.WB), WB(tc_.WB), rec_mel(tc_.e->window_mode == OHW_WINDOW_FIXED_RECORDING_MEL) {
    if (stitch) held.resize((size_t)n_win);
  }
  // ohw_stitch_plan_host's count: with the hop at 480 000 it is ceil(n / 480 000)
  static int64_t share_of(int64_t n, int64_t first, int64_t step, int64_t hop) {
    const int64_t all = n <= 0 ? 0 : n <= CHUNK_SAMPLES ? 1 : (n - CHUNK_SAMPLES + hop - 1) / hop + 1;
    return all > first ? (all - first + step - 1) / step : 0;
  }
  int64_t rec_win(int64_t k) const { return win_first + k * win_step; }
  int32_t win_samples(int64_t k) const { return (int32_t)std::min<int64_t>(CHUNK_SAMPLES, n - rec_win(k) * hop); }
  double win_t_off(int64_t k) const { return (double)rec_win(k) * ((double)hop / 16000.0); }
  int batch_of(int64_t bi) const { return (int)std::min<int64_t>(WB, n_win - bi * WB); }
  void fill_ns(int64_t w0, int B, std::vector<int32_t>& nsv) const { for (int b = 0; b < B; ++b) nsv[(size_t)b] = win_samples(w0 + b); }
  // windows w0 .. w0 + B of the engine's share into st
  void mel_windows(ohw_state* st, int64_t w0, int B, const int32_t* nsv) const {
    if (!rec_mel && hop < CHUNK_SAMPLES) {
      // overlapped windows share samples and ohw_mel takes rows that do not: the batch's windows side by side in a staging
      // buffer of the state's own, which stands until the state's next front end (its decode has been read back by then)
      std::vector<float>& rows = staged[st];
      rows.resize(std::max(rows.size(), (size_t)B * CHUNK_SAMPLES));
      for (int b = 0; b < B; ++b) std::memcpy(&rows[(size_t)b * CHUNK_SAMPLES], samples + rec_win(w0 + b) * hop, (size_t)nsv[b] * 4);
      check(ohw_mel(st, rows.data(), CHUNK_SAMPLES, nsv, B, 0, OHW_MEL_ZERO_TAIL, nullptr));
      return;
    }
    if (!rec_mel) { check(ohw_mel(st, samples + rec_win(w0) * hop, win_step * hop, nsv, B, 0, OHW_MEL_ZERO_TAIL, nullptr)); return; }
    std::vector<int32_t> seeks((size_t)B);
    for (int b = 0; b < B; ++b) seeks[(size_t)b] = (int32_t)(rec_win(w0 + b) * (hop / HOP));
    check(ohw_mel_seek(st, seeks.data(), B, nullptr));
  }
  void front(int64_t bi, ohw_state* st, void* stream, std::vector<int32_t>& nsv) const {
    fill_ns(bi * WB, batch_of(bi), nsv);
    check(ohw_state_set_stream(st, stream));
    mel_windows(st, bi * WB, batch_of(bi), nsv.data());
    check(ohw_encode(st, batch_of(bi)));
  }
  void collect(Scratch& sc, int B, int64_t w0) const {
    tc.flush_trace(sc);
    for (int b = 0; b < B; ++b) {
      if (stitch) { held[(size_t)(w0 + b)] = std::move(sc.runs[(size_t)b]); continue; }
      const double t_off = win_t_off(w0 + b);
      tc.emit(sc.runs[(size_t)b], t_off, std::min(t_off + 30.0, (double)n / 16000.0), e->last, e->prompt);
    }
  }
  // stitched windows, after the last batch: the windows' text tokens, the seams in one launch, the ranges, then every window's
  // records in window order, cut to its range
  void finish() const {
    if (!stitch) return;
    const int W = (int)n_win, stride = tc.max_tok;
    std::vector<int32_t> text((size_t)std::max(W, 1) * stride, 0), nt((size_t)W, 0), t_first((size_t)W, 0), t_end((size_t)W, 0);
    std::vector<std::vector<int>> tpos((size_t)W);         // kept-token position of every text token
    e->last_win_offsets.assign(1, 0);
    for (int w = 0; w < W; ++w) {
      const WindowRun& r = held[(size_t)w];
      const int keep = kept_tokens(r, tc.pol);
      for (int i = 0; i < keep; ++i)
        if (r.tok[(size_t)i] < tc.tk.eot && nt[(size_t)w] < stride) { text[(size_t)w * stride + nt[(size_t)w]++] = r.tok[(size_t)i]; tpos[(size_t)w].push_back(i); }
      e->last_win_tokens.insert(e->last_win_tokens.end(), r.tok.begin(), r.tok.begin() + keep);
      e->last_win_offsets.push_back((int32_t)e->last_win_tokens.size());
    }
    e->last_seams.assign((size_t)std::max(0, W - 1), ohw_seam{});
    check(ohw_stitch_seams(e->device, text.data(), stride, nt.data(), W, e->last_seams.data()));
    check(ohw_stitch_ranges_host(e->last_seams.data(), nt.data(), W, t_first.data(), t_end.data()));
    const double rec_end = (double)n / 16000.0;
    for (int w = 0; w < W; ++w) {
      const WindowRun& r = held[(size_t)w];
      const int keep = kept_tokens(r, tc.pol), rc = t_first[(size_t)w], lc = t_end[(size_t)w];
      // text-token indices to kept-token positions: an uncut end keeps its timestamp tokens
      auto pos = [&](int t, bool is_end) { return (t == 0 && !is_end) ? 0 : t >= nt[(size_t)w] ? keep : tpos[(size_t)w][(size_t)t]; };
      const double t_off = win_t_off(w), t_end_w = std::min(t_off + 30.0, rec_end);
      // the middle of the audio two neighbours share: (start of the right window + end of the left one) / 2
      TranscribeCall::Cut cut{pos(rc, false), pos(lc, true), 0.f, 0.f};
      cut.end = std::max(cut.end, cut.first);
      if (w > 0) cut.t_left = (float)((t_off + std::min(win_t_off(w - 1) + 30.0, rec_end)) / 2.0);
      if (w + 1 < W) cut.t_right = (float)((win_t_off(w + 1) + t_end_w) / 2.0);
      tc.emit(r, t_off, t_end_w, e->last, e->prompt, &cut);
    }
    held.clear();
  }
  void restore_streams() const {
    for (ohw_state* st : e->states) (void)ohw_state_set_stream(st, nullptr);
    for (ohw_state* st : e->lane_states) (void)ohw_state_set_stream(st, nullptr);
    (void)ohw_state_set_stream(e->state, nullptr);
  }
  void sequential() const {
    Scratch sc(WB, tc.max_tok);
    std::vector<int32_t> ns((size_t)WB);
    for (int64_t bi = 0; bi < n_batches; ++bi) {
      fill_ns(bi * WB, batch_of(bi), ns);
      mel_windows(e->state, bi * WB, batch_of(bi), ns.data());
      check(ohw_encode(e->state, batch_of(bi)));
      tc.decode_windows(sc, e->state, bi * WB, batch_of(bi), ns.data());
      collect(sc, batch_of(bi), bi * WB);
    }
  }
  // mel + encoder + cross-K/V of batch i+1 (MFMA-bound) run beside the greedy decode of batch i (HBM- and latency-bound) on
  // disjoint CUs; the first front end and the last decode have the device to themselves
  void pipeline() const {
    Scratch sc(e->max_batch, tc.max_tok);
    std::vector<int32_t> ns2[2] = {std::vector<int32_t>((size_t)e->max_batch), std::vector<int32_t>((size_t)e->max_batch)};
    try {
      front(0, e->states[0], e->s_full, ns2[0]);
      void* last_front = e->s_full;
      for (int64_t bi = 0; bi < n_batches; ++bi) {
        const bool more = bi + 1 < n_batches;
        void* dstream = more ? e->s_dec : e->s_full;
        check(ohw_stream_wait(dstream, last_front));            // this batch's cross-K/V before its decode
        if (more) {
          check(ohw_stream_wait(e->s_enc, last_front));
          front(bi + 1, e->states[(bi + 1) & 1], e->s_enc, ns2[(bi + 1) & 1]);
          last_front = e->s_enc;
        }
        check(ohw_state_set_stream(e->states[bi & 1], dstream));
        tc.decode_windows(sc, e->states[bi & 1], bi * WB, batch_of(bi), ns2[bi & 1].data());
        collect(sc, batch_of(bi), bi * e->max_batch);
      }
    } catch (...) {
      (void)hipDeviceSynchronize();
      restore_streams();
      throw;
    }
    restore_streams();
  }
  // LANES: groups of up to L lanes, each lane up to `merge` batches of max_batch windows.  The lanes' front ends (one
  // pass over all of a lane's windows each) run one after the other on every CU (MFMA-bound: nothing to gain from
  // sharing the chip); a lane decodes its windows as ONE batch (the decoder streams its weights once per step whatever
  // its batch); the L decodes run side by side, each on its own CU-masked stream driven by its own host thread - a
  // decode alternates an HBM-bound kernel (cross-attention) with a chain of latency-bound ones, and several together
  // keep HBM busy (tools/decode_overlap_probe.py).  The kernels' arithmetic does not depend on the CU budget or on a
  // window's batch neighbours, so the results equal the sequential schedule's.  The lane threads share tc, which is
  // constant for the call; each has its own Scratch, state and stream
  void lanes() const {
    const int L = std::max(1, (int)std::min(e->lane_states.size(), e->lane_streams.empty() ? (size_t)1 : e->lane_streams.size()));
    const int merge = std::max(1, std::min(e->merge, e->lane_capacity / std::max(1, e->max_batch)));
    const int64_t DBw = (int64_t)e->max_batch * merge;                  // capacity of a lane's decode batch, windows
    std::vector<std::unique_ptr<Scratch>> scs;
    std::vector<std::vector<int32_t>> nss((size_t)L, std::vector<int32_t>((size_t)DBw));
    for (int i = 0; i < L; ++i) scs.emplace_back(new Scratch((int)DBw, tc.max_tok));
    try {
      // a group = up to L * merge front-end batches, dealt to the lanes as evenly as they go (4 batches on 4 lanes are 4
      // decode batches of one front end each, not one lane with all four)
      for (int64_t b0 = 0; b0 < n_batches;) {
        const int gb = (int)std::min<int64_t>((int64_t)L * merge, n_batches - b0);
        const int grp = std::min(L, gb);
        std::vector<int64_t> lane_w0((size_t)grp);
        std::vector<int> lane_w((size_t)grp);
        int64_t bnext = b0;
        for (int j = 0; j < grp; ++j) {
          const int mj = gb / grp + (j < gb % grp ? 1 : 0);
          lane_w0[(size_t)j] = bnext * e->max_batch;
          lane_w[(size_t)j] = (int)(std::min<int64_t>(n_win, (bnext + mj) * e->max_batch) - lane_w0[(size_t)j]);
          bnext += mj;
        }
        b0 = bnext;
        for (int j = 0; j < grp; ++j) {
          ohw_state* st = e->lane_states[(size_t)j];
          check(ohw_state_set_stream(st, e->s_full));
          // ONE front-end pass over all the lane's windows (its state holds them): the encoder's GEMMs run in rounds of
          // 256 tiles of 256 rows, and 96 windows (563 row tiles) fill their last round where 32 (188) leave it 2/3 empty
          fill_ns(lane_w0[(size_t)j], lane_w[(size_t)j], nss[(size_t)j]);
          mel_windows(st, lane_w0[(size_t)j], lane_w[(size_t)j], nss[(size_t)j].data());
          check(ohw_encode(st, lane_w[(size_t)j]));
        }
        if (grp == 1) {
          tc.decode_windows(*scs[0], e->lane_states[0], lane_w0[0], lane_w[0], nss[0].data());
          collect(*scs[0], lane_w[0], lane_w0[0]);
          continue;
        }
        std::vector<std::string> errs((size_t)grp);
        std::vector<std::thread> th;
        // the host waits for the group's front ends before the lane threads start: lanes that begin to enqueue their
        // decode while the front ends still run cost 6 % of a step in bench.py (283.9 against 262 - 268 ms)
        check(ohw_stream_sync(e->s_full));
        for (int j = 0; j < grp; ++j) {
          check(ohw_stream_wait(e->lane_streams[(size_t)j], e->s_full));
          check(ohw_state_set_stream(e->lane_states[(size_t)j], e->lane_streams[(size_t)j]));
        }
        for (int j = 0; j < grp; ++j)
          th.emplace_back([&, j] {
            try {
              tc.decode_windows(*scs[(size_t)j], e->lane_states[(size_t)j], lane_w0[(size_t)j], lane_w[(size_t)j], nss[(size_t)j].data());
            } catch (const std::exception& ex) {
              errs[(size_t)j] = ex.what()[0] ? ex.what() : "unknown error";
            }
          });
        {
          ApiRelease wait_only;        // the lanes take the library's gate themselves (exclusively while one captures its graph)
          for (auto& t : th) t.join();
        }
        for (int j = 0; j < grp; ++j) if (!errs[(size_t)j].empty()) throw Error(OHW_E_TRANSCRIBE, errs[(size_t)j]);
        for (int j = 0; j < grp; ++j) {
          check(ohw_stream_wait(e->s_full, e->lane_streams[(size_t)j]));
          collect(*scs[(size_t)j], lane_w[(size_t)j], lane_w0[(size_t)j]);
        }
      }
    } catch (...) {
      (void)hipDeviceSynchronize();
      restore_streams();
      throw;
    }
    restore_streams();
  }
};

// resources of the overlapped schedules, made when a long input first needs them: more states, CU-masked streams.  Returns the
// schedule that can run: with no CU-masked queues (or no memory for more states) one batch after the other, from now on
int ensure_schedule_resources(ohw_engine* e, int schedule, int64_t n_batches) {
  if (schedule == OHW_SCHEDULE_SEQUENTIAL) return schedule;
  int rc = OHW_OK, total = 0;
  if (hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || total < 2) rc = OHW_E_TRANSCRIBE;
  if (rc == OHW_OK && !e->s_full) rc = ohw_stream_create(e->device, 0, 0, &e->s_full);
  if (e->states.empty()) e->states.assign(1, e->state);
  auto new_state = [&](int windows, bool lane) {
    ohw_state* st = nullptr;
    rc = ohw_state_create(e->ctx, windows, &st);
    if (rc != OHW_OK) return;
    (void)ohw_state_set_packed_encoder(st, e->packed_encoder);
    (void)ohw_state_set_prefill_chunk(st, e->prefill_chunk);
    if (lane) state_set_graph_max_batch(st, 16);      // see engine.hip: a capture on a lane waits for the other lanes' decodes
    (lane ? e->lane_states : e->states).push_back(st);
  };
  if (schedule == OHW_SCHEDULE_PIPELINE) {
    while (rc == OHW_OK && (int)e->states.size() < 2) new_state(e->max_batch, false);
    if (rc == OHW_OK && !e->s_enc) {
      if (e->enc_cus >= total) e->enc_cus = std::max(1, total * 3 / 8);   // a smaller device: the same 3 : 5 split
      rc = ohw_stream_create(e->device, 0, e->enc_cus, &e->s_enc);
      if (rc == OHW_OK) rc = ohw_stream_create(e->device, e->enc_cus, total - e->enc_cus, &e->s_dec);
    }
  }
  if (rc == OHW_OK && schedule == OHW_SCHEDULE_LANES) {
    // LANES: decode batches of up to merge front-end batches (ohw_encode_slice); a lane's state holds what this input can put
    // into one decode batch (cross K/V is 245.76 MB per window at large-v3)
    const int want_lanes = (int)std::min<int64_t>(e->lanes, n_batches);
    const int64_t per_lane = std::min<int64_t>(std::max(1, e->merge), (n_batches + want_lanes - 1) / std::max(1, want_lanes));
    const int need = (int)(e->max_batch * per_lane);
    if (!e->lane_states.empty() && e->lane_capacity < need) {            // a longer input (or another merge factor) than before
      for (ohw_state* st : e->lane_states) ohw_state_free(st);
      e->lane_states.clear();
    }
    if (e->lane_states.empty()) e->lane_capacity = need;
    while (rc == OHW_OK && (int)e->lane_states.size() < want_lanes) new_state(e->lane_capacity, true);
    if (rc == OHW_OK && want_lanes >= 2 && (int)e->lane_streams.size() != want_lanes) {
      for (void* ls : e->lane_streams) (void)ohw_stream_destroy(ls);     // another lane count: other CU ranges
      e->lane_streams.clear();
      const int per = std::max(1, total / want_lanes);
      for (int i = 0; rc == OHW_OK && i < want_lanes; ++i) {
        void* ls = nullptr;
        rc = ohw_stream_create(e->device, i * per, per, &ls);
        if (rc == OHW_OK) e->lane_streams.push_back(ls);
      }
    }
  }
  if (rc != OHW_OK) {
    engine_free_overlap(e);
    e->schedule = schedule = OHW_SCHEDULE_SEQUENTIAL;
  }
  if (schedule == OHW_SCHEDULE_LANES && e->lane_states.empty()) schedule = OHW_SCHEDULE_SEQUENTIAL;
  if (schedule == OHW_SCHEDULE_PIPELINE && (e->states.size() < 2 || !e->s_enc)) schedule = OHW_SCHEDULE_SEQUENTIAL;
  return schedule;
}

// audio longer than one batch: kernel variants no longer picked from a batch's row count, so a window decodes to the
// same bits whichever batch (a short last one, a merged one) and schedule it lands in (include/ohw.h)
struct Invariant {
  ohw_engine* e; bool on;
  void set(bool v) { each_state(e, [&](ohw_state* st) { (void)ohw_state_set_batch_invariant(st, v); }); }
  Invariant(ohw_engine* e_, bool on_) : e(e_), on(on_) { if (on) set(true); }
  ~Invariant() { if (on) set(false); }
};
struct SharedRecording {      // every state of this transcribe reads the recording e->state holds
  ohw_engine* e; bool on;
  SharedRecording(ohw_engine* e_, bool on_) : e(e_), on(on_) {
    if (!on) return;
    for (ohw_state* st : e->states) state_share_recording(st, e->state);
    for (ohw_state* st : e->lane_states) state_share_recording(st, e->state);
  }
  ~SharedRecording() {
    if (!on) return;
    for (ohw_state* st : e->states) if (st != e->state) state_drop_recording(st);
    for (ohw_state* st : e->lane_states) state_drop_recording(st);
  }
};
// the logit rules of the engine's own state (the engine's setters, or the ohw_state_set_* entries on ohw_engine_state(e): a logit
// bias is the engine's form of whisper.cpp's logits_filter_callback) apply to every state a schedule decodes on, or to none.
// This is the one delivery: the other states exist from ensure_schedule_resources on and decode only in this transcribe
void sync_logit_rules(ohw_engine* e) {
  try {
    each_state(e, [&](ohw_state* st) { state_rules(st).sync_from(state_rules(e->state)); });
  } catch (const Error& err) {
    throw Error(OHW_E_TRANSCRIBE, std::string("Transcription failed: ") + err.what());
  }
}

void transcribe_fixed(const TranscribeCall& tc, const float* samples, int64_t n, int64_t win_first, int64_t win_step) {
  ohw_engine* e = tc.e;
  const FixedCuts cuts(tc, samples, n, win_first, win_step);
  const int call_ctx = engine_call_ctx(e, n);
  for (int64_t k = 0; k < cuts.n_win; ++k) check_window_fits(call_ctx, cuts.rec_win(k), cuts.win_samples(k));
  if (cuts.rec_mel) check(ohw_recording_set(e->state, samples, n, 0, nullptr));
  int schedule = cuts.n_batches > 1 ? e->schedule : OHW_SCHEDULE_SEQUENTIAL;
  if (tc.beam_K > 0 || tc.best_N > 1) schedule = OHW_SCHEDULE_SEQUENTIAL;      // no lanes for beams or best-of: the serial path on the engine's own state
  if (schedule == OHW_SCHEDULE_LANES && e->lanes < 2) schedule = OHW_SCHEDULE_SEQUENTIAL;
  if (schedule == OHW_SCHEDULE_PIPELINE && e->enc_cus <= 0) schedule = OHW_SCHEDULE_SEQUENTIAL;
  schedule = ensure_schedule_resources(e, schedule, cuts.n_batches);
  // an engine of a pool that aligns: its share may be one batch while the recording is several, and the alignment's path is
  // sensitive to last bits, so the times must not depend on how the windows were dealt
  // (confidence alike: a score is a function of the last bits of a row)
  Invariant invariant(e, cuts.n_batches > 1 || (cuts.stitch && cuts.n_win > 1) || ((!e->wt_heads.empty() || e->confidence) && win_step > 1));
  SharedRecording shared_recording(e, cuts.rec_mel);
  sync_logit_rules(e);
  apply_ctx(e, call_ctx);
  if (schedule == OHW_SCHEDULE_SEQUENTIAL) cuts.sequential();
  else if (schedule == OHW_SCHEDULE_PIPELINE) cuts.pipeline();
  else cuts.lanes();
  cuts.finish();
}
}  // namespace

namespace ohw {

void engine_transcribe(ohw_engine* e, const float* samples, int64_t n, int64_t win_first, int64_t win_step) {
  if (win_first < 0 || win_step < 1) throw Error(OHW_E_INVALID_ARG, "transcribe: window dealing must be first >= 0, step >= 1");
  const TranscribeCall tc(e, samples, n);
  if (e->window_mode == OHW_WINDOW_SEEK) transcribe_seek(tc, samples, n);
  else transcribe_fixed(tc, samples, n, win_first, win_step);
}

// ohw_engine_transcribe_batch: every recording one window of its own; longest first, max_batch at a time, one batch after the
// other on the engine's own state.  Under the auto setting a batch's envelope is its largest context and every window runs at
// its own (ohw_state_set_window_ctx) - unless all of them equal the envelope, which is the uniform path
// the front end of the short batch, shared with ohw_engine_score_batch: plan, stage, context, mel, encode and languages of one
// batch after the other; then run(bi, B, ord, ns, langs or null) on the engine's own state, whose cross K/V holds the batch
template <typename F>
static void short_batch_front(ohw_engine* e, const TranscribeCall& tc, const ohw_audio_span* recs, int n_recs, const int32_t* rec_langs, const char* what,
                              F&& run) {
  std::vector<int64_t> lens((size_t)n_recs);
  for (int i = 0; i < n_recs; ++i) lens[(size_t)i] = recs[i].n;
  const int MB = tc.WB, n_b = (n_recs + MB - 1) / MB, full_ctx = e->ctx->hp.n_audio_ctx;
  std::vector<int32_t> order((size_t)n_recs), rctx((size_t)n_recs), env((size_t)n_b);
  const int prc = ohw_batch_plan(lens.data(), n_recs, MB, e->audio_ctx, order.data(), rctx.data(), env.data());
  if (prc != OHW_OK) throw Error(prc, g_last_error);
  BatchStateGuard restore_state(e, true);
  std::vector<float> stage;
  std::vector<int32_t> ns((size_t)MB), wl((size_t)MB), batch_lang;
  // a language per recording: the caller's ids, or a detection per recording when the engine detects; an English-only model
  // has no language token and stays as it is
  const bool per_rec = tc.V >= 51865 && (rec_langs != nullptr || engine_detects(e));
  check_recording_langs(what, rec_langs, n_recs, tc.tk.n_langs);
  for (int bi = 0; bi < n_b; ++bi) {
    const int B = std::min(MB, n_recs - bi * MB);
    const int32_t* ord = &order[(size_t)bi * MB];
    const int E = std::min<int>(env[(size_t)bi], full_ctx);
    bool ragged = false;
    for (int b = 0; b < B; ++b) {
      ns[(size_t)b] = (int32_t)recs[ord[b]].n;
      wl[(size_t)b] = std::min<int>(rctx[(size_t)ord[b]], full_ctx);
      ragged = ragged || wl[(size_t)b] != E;
    }
    const int64_t stride = ns[0];       // the longest of the batch
    stage.assign((size_t)(stride * B), 0.0f);
    for (int b = 0; b < B; ++b) std::memcpy(&stage[(size_t)(stride * b)], recs[ord[b]].samples, (size_t)ns[(size_t)b] * sizeof(float));
    check(ohw_state_set_audio_ctx(e->state, E));
    check(ohw_state_set_window_ctx(e->state, ragged ? wl.data() : nullptr, ragged ? B : 0));
    check(ohw_mel(e->state, stage.data(), stride, ns.data(), B, 0, OHW_MEL_ZERO_TAIL, nullptr));
    check(ohw_encode(e->state, B));
    if (per_rec) {
      batch_lang.assign((size_t)B, OHW_LANG_DETECT);
      for (int b = 0; rec_langs && b < B; ++b) batch_lang[(size_t)b] = rec_langs[ord[b]];
      apply_window_langs(e->state, batch_lang, true);
    }
    run(bi, B, ord, ns.data(), per_rec ? batch_lang.data() : nullptr);
  }
}

void engine_transcribe_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, const int32_t* rec_langs, const double* t_offs, bool trim) {
  const TranscribeCall tc(e, nullptr, 0);
  e->batch_records.assign((size_t)n_recs, ohw_engine::BatchRecord());
  const int MB = tc.WB;
  Scratch sc(MB, tc.max_tok);
  short_batch_front(e, tc, recs, n_recs, rec_langs, "transcribe_batch", [&](int bi, int B, const int32_t* ord, const int32_t* ns, const int32_t* batch_lang) {
    tc.decode_windows(sc, e->state, (int64_t)bi * MB, B, ns, batch_lang);
    sc.trace.clear();
    sc.cands.clear();
    for (int b = 0; b < B; ++b) {
      ohw_engine::BatchRecord& r = e->batch_records[(size_t)ord[b]];
      const double t_off = t_offs ? t_offs[ord[b]] : 0.0;
      tc.emit(sc.runs[(size_t)b], t_off, t_off + (double)recs[ord[b]].n / 16000.0, r.t, e->prompt);
      if (trim) r.t.trim();
      r.lang_id = batch_lang ? batch_lang[b] : -1;
    }
  });
}

// ohw_engine_score_batch: the short batch's front end, then ohw_state_score on the caller's tokens instead of a decode
void engine_score_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, const int32_t* tokens, const int32_t* offsets, ohw_score_result* results) {
  const TranscribeCall tc(e, nullptr, 0);
  const int half = tc.max_tok / 2, MB = tc.WB;
  for (int i = 0; i < n_recs; ++i) {
    const int64_t nt = (int64_t)offsets[i + 1] - offsets[i];
    if (offsets[i] < 0 || nt < 0 || nt > half)
      throw Error(OHW_E_INVALID_ARG, "score_batch: recording " + std::to_string(i) + " has " + std::to_string(nt) + " tokens, outside 0 .. n_text_ctx / 2 = " + std::to_string(half));
    for (int64_t k = 0; k < nt; ++k)
      if (tokens[offsets[i] + k] < 0 || tokens[offsets[i] + k] >= tc.tk.eot)
        throw Error(OHW_E_INVALID_ARG, "score_batch: recording " + std::to_string(i) + ", token " + std::to_string(k) + ": id " + std::to_string(tokens[offsets[i] + k]) +
                                           " is not a text token (0 .. " + std::to_string(tc.tk.eot - 1) + ")");
  }
  e->score_records.assign((size_t)n_recs, std::vector<ohw_token_prob>());
  const float nan = __builtin_nanf("");
  std::vector<int32_t> atok((size_t)MB * half), nt((size_t)MB);
  std::vector<ohw_token_score> scores((size_t)MB * (half + 1));
  short_batch_front(e, tc, recs, n_recs, nullptr, "score_batch", [&](int, int B, const int32_t* ord, const int32_t*, const int32_t*) {
    bool any = false;
    for (int b = 0; b < B; ++b) {
      nt[(size_t)b] = offsets[ord[b] + 1] - offsets[ord[b]];
      std::copy(tokens + offsets[ord[b]], tokens + offsets[ord[b] + 1], atok.begin() + (long)((size_t)b * half));
      any = any || nt[(size_t)b] > 0;
    }
    if (any) check(ohw_state_score(e->state, &tc.sp, atok.data(), half, nt.data(), B, scores.data(), nullptr, nullptr));
    for (int b = 0; b < B; ++b) {
      const int i = ord[b], n = nt[(size_t)b];
      std::vector<ohw_token_prob>& rec = e->score_records[(size_t)i];
      ohw_score_result& r = results[i];
      r.eot = ohw_token_prob{tc.tk.eot, 0, nan, nan, nan, -1, nan};
      r.sum_logprob_all = nan;
      double sum = 0.0;
      for (int k = 0; n > 0 && k <= n; ++k) {
        const ohw_token_score& s = scores[(size_t)b * (half + 1) + k];
        ohw_token_prob tp{k < n ? atok[(size_t)b * half + k] : tc.tk.eot, 0, 0.f, 0.f, nan, s.top_id, 0.f};
        (void)ohw_token_prob_host(&s, &tp.logprob_text, &tp.logprob_all, &tp.top_logprob_text);
        sum += tp.logprob_all;
        if (k < n) rec.push_back(tp); else r.eot = tp;
      }
      if (n > 0) r.sum_logprob_all = (float)sum;
    }
  });
  for (int i = 0; i < n_recs; ++i) { results[i].tokens = e->score_records[(size_t)i].data(); results[i].n_tokens = (int32_t)e->score_records[(size_t)i].size(); }
}

// ohw_engine_transcribe_speech: the front half (detector, segments, chunks) per recording, then every chunk of every recording as
// one recording of ONE engine_transcribe_batch - emitted with its offset on its recording's clock - and the chunk records
// appended to their recording's, the way the fixed-cut path appends its windows
void engine_transcribe_speech(ohw_engine* e, const ohw_audio_span* recs, const ohw_frame_probs* probs, int n_recs, const int32_t* rec_langs) {
  std::vector<ohw_engine::BatchRecord> out((size_t)n_recs);
  std::vector<ohw_audio_span> pool;
  std::vector<double> offs;
  std::vector<int32_t> pool_lang, owner;
  std::vector<float> own;
  for (int i = 0; i < n_recs; ++i) {
    const int64_t n = recs[i].n;
    const float* p = probs ? probs[i].p : nullptr;
    int64_t n_p = probs ? probs[i].n : 0;
    int fs = probs ? probs[i].frame_samples : 0;
    if (!p || n_p <= 0) {                               // the device detector, 10 ms frames
      n_p = (n + HOP - 1) / HOP; fs = HOP;
      own.assign((size_t)n_p, 0.0f);
      check(ohw_state_vad_frames(e->state, recs[i].samples, n, 0, &e->vad_det, own.data(), nullptr));
      p = own.data();
    } else if (fs < 1) {
      throw Error(OHW_E_INVALID_ARG, "transcribe_speech: recording " + std::to_string(i) + " has probabilities with frame_samples < 1");
    }
    ohw_engine::BatchRecord& r = out[(size_t)i];
    r.per_window = true;
    r.speech.resize((size_t)n_p / 2 + 1);               // a segment needs a frame at or above the threshold and one below behind it
    const int64_t n_seg = ohw_speech_segments_host(p, n_p, fs, n, &e->vad_cfg, r.speech.data(), (int64_t)r.speech.size());
    if (n_seg < 0 || n_seg > (int64_t)r.speech.size()) throw Error(OHW_E_INVALID_ARG, "transcribe_speech: bad probabilities or vad settings for recording " + std::to_string(i));
    r.speech.resize((size_t)n_seg);
    const int64_t n_ch = ohw_speech_chunks_host(r.speech.data(), n_seg, p, n_p, fs, n, &e->chunk_plan, nullptr, 0);
    if (n_ch < 0) throw Error(OHW_E_INVALID_ARG, "transcribe_speech: bad chunk plan for recording " + std::to_string(i));
    r.chunks.resize((size_t)n_ch);
    (void)ohw_speech_chunks_host(r.speech.data(), n_seg, p, n_p, fs, n, &e->chunk_plan, r.chunks.data(), n_ch);
    for (const ohw_speech_chunk& c : r.chunks) {
      pool.push_back(ohw_audio_span{recs[i].samples + c.start, c.end - c.start});
      offs.push_back((double)c.start / 16000.0);
      owner.push_back(i);
      if (rec_langs) pool_lang.push_back(rec_langs[i]);
    }
  }
  if (!pool.empty()) {
    if (pool.size() > (size_t)0x7fffffff) throw Error(OHW_E_INVALID_ARG, "transcribe_speech: too many chunks");
    engine_transcribe_batch(e, pool.data(), (int)pool.size(), rec_langs ? pool_lang.data() : nullptr, offs.data(), false);
    for (size_t k = 0; k < pool.size(); ++k) {
      ohw_engine::BatchRecord& r = out[(size_t)owner[k]];
      const Transcript& c = e->batch_records[k].t;
      Transcript& t = r.t;
      const size_t text0 = t.text.size();
      const int32_t win0 = (int32_t)t.quality.size();
      if (win0 == 0) r.lang_id = e->batch_records[k].lang_id;          // a recording reports its first chunk's language
      t.text += c.text;
      t.tokens.insert(t.tokens.end(), c.tokens.begin(), c.tokens.end());
      t.quality.insert(t.quality.end(), c.quality.begin(), c.quality.end());
      for (ohw_token_time tt : c.token_times) { tt.window += win0; t.token_times.push_back(tt); }
      for (ohw_span_time w : c.words) { w.text_off += text0; t.words.push_back(w); }
      for (ohw_span_time sg : c.segments) { sg.text_off += text0; t.segments.push_back(sg); }
      for (ohw_token_prob tp : c.token_probs) { tp.window += win0; t.token_probs.push_back(tp); }
      for (ohw_word_prob wp : c.word_probs) { wp.text_off += text0; t.word_probs.push_back(wp); }
      t.segment_info.insert(t.segment_info.end(), c.segment_info.begin(), c.segment_info.end());
      for (WindowMark m : c.marks) { m.text0 += text0; t.marks.push_back(m); }
      t.contexts.insert(t.contexts.end(), c.contexts.begin(), c.contexts.end());
      for (ohw_command_hit hit : c.commands) { hit.window += win0; t.commands.push_back(hit); }
    }
  } else {
    const TranscribeCall tc(e, nullptr, 0);             // what every call starts with: the last call's records are gone
    check_recording_langs("transcribe_speech", rec_langs, n_recs, tc.tk.n_langs);
  }
  for (ohw_engine::BatchRecord& r : out) r.t.trim();
  e->batch_records = std::move(out);
}

// ohw_engine_transcribe_long_batch: the seek loop of every recording, one window of each live recording per round, on the
// engine's own state.  Each recording is one whisper_full call: its own generator across all its windows, its own frame count as
// the end of the audio, the full audio context (what the single loop runs anything longer than a window at).  The generator and
// the carried history follow the recording, not the slot: a refilled slot starts from its new recording's own
void engine_transcribe_long_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, const int32_t* rec_langs) {
  const TranscribeCall tc(e, nullptr, 0);
  e->batch_records.assign((size_t)n_recs, ohw_engine::BatchRecord());
  const int MB = tc.WB;
  std::vector<int64_t> lens((size_t)n_recs);
  for (int i = 0; i < n_recs; ++i) lens[(size_t)i] = recs[i].n;
  ohw_seek_sched* sched = nullptr;
  const int src = ohw_seek_sched_new(lens.data(), n_recs, MB, &sched);
  if (src != OHW_OK) throw Error(src, g_last_error);
  struct SchedFree { ohw_seek_sched* s; ~SchedFree() { ohw_seek_sched_free(s); } } sched_free{sched};
  BatchStateGuard restore_state(e, false);
  const bool per_rec = tc.V >= 51865 && (rec_langs != nullptr || engine_detects(e));
  check_recording_langs("transcribe_long_batch", rec_langs, n_recs, tc.tk.n_langs);
  check(ohw_state_set_stream(e->state, nullptr));
  check(ohw_state_set_audio_ctx(e->state, 0));
  check(ohw_state_set_window_ctx(e->state, nullptr, 0));
  // a recording's language: the caller's id, or OHW_LANG_DETECT until its first window has been detected (with no table: -1)
  std::vector<int32_t> rec_lang((size_t)n_recs, -1), batch_lang;
  if (per_rec) for (int i = 0; i < n_recs; ++i) rec_lang[(size_t)i] = rec_langs ? rec_langs[i] : OHW_LANG_DETECT;
  const int N = tc.best_N;
  Rngs rngs((size_t)n_recs, N);
  std::vector<Carry> carry((size_t)(tc.carrying ? n_recs : 0));
  for (Carry& c : carry) tc.carry_init(c);
  Scratch sc(MB, tc.max_tok);
  std::vector<int32_t> r_rec((size_t)MB), r_slot((size_t)MB), r_seek((size_t)MB), r_fresh((size_t)MB);
  std::vector<int> seeks((size_t)MB), ends((size_t)MB), frames((size_t)MB);
  std::vector<ohw_rng*> round_rngs((size_t)MB * (size_t)N);
  std::vector<const std::vector<int32_t>*> round_ctx((size_t)MB, nullptr);
  for (;;) {
    const int B = ohw_seek_sched_round(sched, r_rec.data(), r_slot.data(), r_seek.data(), r_fresh.data());
    if (B < 0) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: " + g_last_error);
    if (B == 0) break;
    for (int b = 0; b < B; ++b) {
      const int i = r_rec[(size_t)b];
      if (r_fresh[(size_t)b]) check(ohw_recording_set_slot(e->state, r_slot[(size_t)b], recs[i].samples, recs[i].n, 0, nullptr));
      seeks[(size_t)b] = r_seek[(size_t)b];
      ends[(size_t)b] = mel_frames(recs[i].n);
      frames[(size_t)b] = std::min(CHUNK_FRAMES, ends[(size_t)b] - seeks[(size_t)b]);
      for (int j = 0; j < N; ++j) round_rngs[(size_t)(b * N + j)] = rngs.v[(size_t)(i * N + j)];
      if (tc.carrying) round_ctx[(size_t)b] = &carry[(size_t)i].next;
    }
    check(ohw_mel_seek_slots(e->state, r_slot.data(), r_seek.data(), B, nullptr));
    check(ohw_encode(e->state, B));
    if (per_rec) {
      batch_lang.resize((size_t)B);
      for (int b = 0; b < B; ++b) batch_lang[(size_t)b] = rec_lang[(size_t)r_rec[(size_t)b]];
      // whisper.cpp detects once per whisper_full call, on the first window: read back once, kept for the later windows
      if (apply_window_langs(e->state, batch_lang, false))
        for (int b = 0; b < B; ++b) rec_lang[(size_t)r_rec[(size_t)b]] = batch_lang[(size_t)b];
    }
    const Batch bt{e->state, B, seeks.data(), ends.data(), 0, per_rec ? batch_lang.data() : nullptr, tc.carrying ? round_ctx.data() : nullptr, round_rngs.data()};
    tc.pass_t0(sc, bt);
    tc.run_ladder(sc, bt);
    tc.align_runs(sc, e->state, B, frames.data());
    sc.trace.clear();
    sc.cands.clear();
    for (int b = 0; b < B; ++b) {
      const int i = r_rec[(size_t)b];
      const WindowRun& r = sc.runs[(size_t)b];
      tc.emit(r, seeks[(size_t)b] * 0.01, std::min(seeks[(size_t)b] * 0.01 + 30.0, (double)recs[i].n / 16000.0), e->batch_records[(size_t)i].t,
              tc.carrying ? *round_ctx[(size_t)b] : e->prompt);
      if (tc.carrying) tc.carry_step(carry[(size_t)i], &r);
      check(ohw_seek_sched_advance(sched, b, r.ev.seek_delta));
    }
  }
  if (tc.carrying) check(ohw_state_set_window_prompt(e->state, nullptr, 0, nullptr, 0));
  for (int i = 0; i < n_recs; ++i) {
    ohw_engine::BatchRecord& r = e->batch_records[(size_t)i];
    r.t.trim();
    r.per_window = true;
    // a recording that never ran a window (under 1 s) was never detected: id 0, as the single loop reports it
    r.lang_id = !per_rec ? -1 : rec_lang[(size_t)i] == OHW_LANG_DETECT ? 0 : rec_lang[(size_t)i];
  }
}

}  // namespace ohw
