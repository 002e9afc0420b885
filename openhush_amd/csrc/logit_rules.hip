// logit_rules.hip — LogitRules (logit_rules.hpp): the setters, the device order (apply), its host twin (apply_host) and the sync
// between the states of an engine.  The kernels and their host twins live in phrase.hip, repeat.hip and command.hip.
#include "logit_rules.hpp"

#include <cmath>
#include <cstring>
#include <limits>

namespace ohw {

void LogitRules::set_bias(const float* values, int n) {
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipStreamSynchronize(*stream));
  if (!values) { bias.on = false; bias.host.clear(); return; }
  if (n != n_vocab) throw Error(OHW_E_INVALID_ARG, "logit bias: n must equal n_vocab");
  // -inf means "never" (the samplers give such an entry probability 0); +inf and NaN would poison a row's log-sum-exp
  for (int i = 0; i < n; ++i)
    if (std::isnan(values[i]) || values[i] == INFINITY) throw Error(OHW_E_INVALID_ARG, "logit bias: entry " + std::to_string(i) + " is +inf or NaN");
  if (!bias.dev.p) bias.dev.alloc((size_t)n * 4);
  HIP_CHECK(hipMemcpy(bias.dev.p, values, (size_t)n * 4, hipMemcpyHostToDevice));
  bias.host.assign(values, values + n);
  bias.on = true;
}

void LogitRules::upload_phrases(const ohw_phrase_table* t, int table_vocab) {
  std::vector<int32_t> words;
  phrase_table_pack(t, table_vocab, &words);
  if (!ph.table.p) ph.table.alloc((size_t)PH_WORDS * 4, true);
  HIP_CHECK(hipMemcpy(ph.table.p, words.data(), words.size() * 4, hipMemcpyHostToDevice));
}

void LogitRules::set_phrases(const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases) {
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipStreamSynchronize(*stream));
  if (n_phrases == 0) { ph.on = false; return; }
  // built aside first: a refused table leaves the one in effect as it was
  std::vector<int32_t> child_off((size_t)OHW_PHRASE_MAX_NODES + 1), path((size_t)OHW_PHRASE_MAX_PATH), child_tok((size_t)OHW_PHRASE_MAX_EDGES);
  std::vector<float> child_boost((size_t)OHW_PHRASE_MAX_EDGES);
  ohw_phrase_table t{};
  t.child_off = child_off.data(); t.path = path.data(); t.child_tok = child_tok.data(); t.child_boost = child_boost.data();
  phrase_table_build_host(tokens, offsets, boosts, n_phrases, eot, &t);
  upload_phrases(&t, n_vocab);
  ph.child_off.swap(child_off); ph.path.swap(path); ph.child_tok.swap(child_tok); ph.child_boost.swap(child_boost);
  ph.host = t;                                         // the vectors' storage moved with the swap: the pointers hold
  ph.src_tok.assign(tokens, tokens + offsets[n_phrases]);
  ph.src_off.assign(offsets, offsets + n_phrases + 1);
  ph.src_boost.assign(boosts, boosts + n_phrases);
  ph.on = true;
}

void LogitRules::upload_repeat(float penalty, int ngram) {
  int32_t words[2];
  std::memcpy(&words[0], &penalty, 4);
  words[1] = ngram;
  if (!rp.rule.p) rp.rule.alloc(sizeof words, true);
  HIP_CHECK(hipMemcpy(rp.rule.p, words, sizeof words, hipMemcpyHostToDevice));
}

void LogitRules::set_repeat(float penalty, int ngram) {
  repeat_rule_check(penalty, ngram);                   // the values first: a refusal needs no device
  const bool on = penalty != 1.0f || ngram != 0;
  if (on || rp.rule.p) {                               // a state that never had the rule on owns no buffer and needs none
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamSynchronize(*stream));
    upload_repeat(penalty, ngram);
  }
  rp.penalty = penalty; rp.ngram = ngram; rp.on = on;
}

void LogitRules::upload_commands(const ohw_command_table* t, float penalty) {
  std::vector<int32_t> words;
  command_table_pack(t, penalty, &words);
  if (!cm.table.p) cm.table.alloc((size_t)CM_WORDS * 4, true);
  if (!cm.lp.p) {
    const std::vector<float> nan((size_t)max_batch, std::numeric_limits<float>::quiet_NaN());
    cm.lp.alloc(nan.size() * 4, true);
    HIP_CHECK(hipMemcpy(cm.lp.p, nan.data(), nan.size() * 4, hipMemcpyHostToDevice));
  }
  HIP_CHECK(hipMemcpy(cm.table.p, words.data(), words.size() * 4, hipMemcpyHostToDevice));
}

void LogitRules::set_commands(const int32_t* tokens, const int32_t* offsets, int n_phrases, float penalty) {
  if (n_phrases != 0) command_penalty_check(penalty);  // the value first: a refusal needs no device
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipStreamSynchronize(*stream));
  if (n_phrases == 0) { cm.on = false; return; }
  // built aside first: a refused list leaves the one in effect as it was
  std::vector<int32_t> child_off((size_t)OHW_COMMAND_MAX_NODES + 1), path((size_t)OHW_COMMAND_MAX_PATH), child_tok((size_t)OHW_COMMAND_MAX_EDGES),
      terminal((size_t)OHW_COMMAND_MAX_NODES), phrase_id((size_t)OHW_COMMAND_MAX_NODES);
  ohw_command_table t{};
  t.child_off = child_off.data(); t.path = path.data(); t.child_tok = child_tok.data(); t.terminal = terminal.data(); t.phrase_id = phrase_id.data();
  command_table_build_host(tokens, offsets, n_phrases, eot, &t);
  upload_commands(&t, penalty);
  cm.child_off.swap(child_off); cm.path.swap(path); cm.child_tok.swap(child_tok); cm.terminal.swap(terminal); cm.phrase_id.swap(phrase_id);
  cm.host = t;                                         // the vectors' storage moved with the swap: the pointers hold
  cm.src_tok.assign(tokens, tokens + offsets[n_phrases]);
  cm.src_off.assign(offsets, offsets + n_phrases + 1);
  cm.penalty = penalty;
  cm.on = true;
}

void LogitRules::list_logprob(int batch, float* out) const {
  if (!cm.on) throw Error(OHW_E_INVALID_ARG, "command list: none is set on this state");
  if (batch < 1 || batch > max_batch) throw Error(OHW_E_INVALID_ARG, "command list: batch must lie in 1..max_batch");
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipStreamSynchronize(*stream));
  HIP_CHECK(hipMemcpy(out, cm.lp.p, (size_t)batch * 4, hipMemcpyDeviceToHost));
}

void LogitRules::apply(float* logits, int64_t ld, const SamplerParams& p, int rows, int row_mul, int group, const int32_t* n_cur, const int32_t* done,
                       hipStream_t s, int lp_group) {
  if (ph.on) {
    PhraseBoostParams b{};
    b.logits = logits; b.ld = ld; b.n_vocab = p.n_vocab; b.max_tokens = p.max_tokens; b.row_mul = row_mul; b.group = group;
    b.tokens = p.tokens; b.n_cur = n_cur; b.done = done; b.table = ph.table.as<int32_t>();
    launch_phrase_boost(b, rows, s);
    ++tally_phrase;
  }
  // null n_cur is the group pass's first step, where every history is empty by definition: the launch is skipped.  The beam's
  // first step passes the windows' n_cur, which the device holds as zeros: there the kernel runs and returns at once
  if (rp.on && n_cur) {
    RepeatRuleParams q{};
    q.logits = logits; q.ld = ld; q.n_vocab = p.n_vocab; q.max_tokens = p.max_tokens; q.row_mul = row_mul; q.group = group;
    q.eot = p.eot; q.tokens = p.tokens; q.n_cur = n_cur; q.done = done; q.rule = rp.rule.as<int32_t>();
    launch_repeat_rule(q, rows, s);
    ++tally_repeat;
  }
  // null n_cur launches here: the first step is where the root applies
  if (cm.on) {
    CommandRuleParams q{};
    q.logits = logits; q.ld = ld; q.n_vocab = p.n_vocab; q.max_tokens = p.max_tokens; q.row_mul = row_mul; q.group = group;
    q.lp_group = lp_group > 0 ? lp_group : group;
    q.eot = p.eot; q.tokens = p.tokens; q.n_cur = n_cur; q.done = done; q.table = cm.table.as<int32_t>(); q.list_logprob = cm.lp.as<float>();
    launch_command_rule(q, rows, s);
    ++tally_command;
  }
}

int LogitRules::apply_host(const int32_t* history, int n, float* row, int n_vocab_, int eot_, float* list_lp) const {
  int rc = OHW_OK;
  if (ph.on) rc = ohw_phrase_boost_host(&ph.host, history, n, row, n_vocab_);
  if (rc == OHW_OK && rp.on) rc = ohw_repeat_rule_host(rp.penalty, rp.ngram, history, n, row, n_vocab_, eot_);
  if (rc == OHW_OK && cm.on) rc = ohw_command_rule_host(&cm.host, cm.penalty, history, n, row, n_vocab_, eot_, list_lp);
  if (rc == OHW_OK && bias.on && !bias.host.empty())
    for (int i = 0; i < n_vocab_; ++i) row[i] += bias.host[(size_t)i];
  return rc;
}

void LogitRules::sync_from(const LogitRules& src) {
  if (this == &src) return;
  auto same = [](const auto& a, const auto& b, size_t n) { return std::memcmp(a.data(), b.data(), n * 4) == 0; };
  // bias: on here or there, and not the same values on both sides
  if ((src.bias.on || bias.on) && !(src.bias.on && bias.on && same(src.bias.host, bias.host, (size_t)n_vocab)))
    set_bias(src.bias.on ? src.bias.host.data() : nullptr, src.bias.on ? n_vocab : 0);
  // hot phrases: the phrases as they were given, with their boosts
  const Phrases& p = src.ph;
  const int np = src.phrase_count();
  if ((np || ph.on) && !(np == phrase_count() && same(p.src_off, ph.src_off, (size_t)np + 1) && same(p.src_tok, ph.src_tok, (size_t)p.src_off[(size_t)np]) &&
                         same(p.src_boost, ph.src_boost, (size_t)np)))
    set_phrases(p.src_tok.data(), p.src_off.data(), p.src_boost.data(), np);
  // repetition rule: the two values
  if (rp.penalty != src.rp.penalty || rp.ngram != src.rp.ngram) set_repeat(src.rp.penalty, src.rp.ngram);
  // command list: the phrases as they were given, and the penalty
  const Commands& c = src.cm;
  const int nc = src.command_count();
  if ((nc || cm.on) && !(nc == command_count() && c.penalty == cm.penalty && same(c.src_off, cm.src_off, (size_t)nc + 1) &&
                         same(c.src_tok, cm.src_tok, (size_t)c.src_off[(size_t)nc])))
    set_commands(c.src_tok.data(), c.src_off.data(), nc, c.penalty);
}

}  // namespace ohw
