// logit_rules.hpp — the four rules that change a row's logits ahead of every sampler, and their one owner per state: the static
// logit bias (the samplers add it themselves), the hot-phrase boost, the repetition rule and the command list.
#pragma once
#include <vector>

#include "kernels.hpp"
#include "model.hpp"

namespace ohw {

// Per rule: the device buffer(s), the host twin, the source as the caller gave it, the on flag.
//
// INVARIANT: a captured step graph holds the raw device pointers of ph.table, rp.rule, cm.table and cm.lp.  So the object is
// neither copied nor moved, a buffer once allocated is never freed or reallocated before the object dies, and sync_from copies
// contents, never buffers.  "Swapping lists or penalties captures nothing" rests on this; that a rule is on is part of the key.
struct LogitRules {
  // set once, by init: what the setters' checks need, and where the owner keeps its current stream (ohw_state_set_stream may
  // change it) - a setter that is going to write a device buffer first waits for the stream whose kernels read it
  int device = 0, n_vocab = 0, eot = 0, max_batch = 0;
  const hipStream_t* stream = nullptr;

  struct Bias {
    DevBuf dev;                      // f32 [n_vocab], made at the first set
    std::vector<float> host;         // the same on the host: the temperature ladder may sample there
    bool on = false;
  } bias;
  // hot phrases: the flat trie in one fixed-size device buffer (kernels.hpp, PH_WORDS), made at the first set; host: the same
  // table with the arrays it points into; src_*: the phrases as they were given
  struct Phrases {
    DevBuf table;
    ohw_phrase_table host{};
    std::vector<int32_t> child_off, path, child_tok, src_tok, src_off;
    std::vector<float> child_boost, src_boost;
    bool on = false;
  } ph;
  // repetition penalty and no-repeat n-grams: the two values, and a two-word device buffer {fp32 bits of the penalty, n-gram
  // size} made at the first set that turns the rule on; on: they are not (1.0, 0)
  struct Repeat {
    DevBuf rule;
    float penalty = 1.0f;
    int ngram = 0;
    bool on = false;
  } rp;
  // command list: the anchored trie and the penalty in one fixed-size device buffer (kernels.hpp, CM_WORDS) and list_logprob
  // [max_batch], both made at the first set; host, src_*: as for the phrases
  struct Commands {
    DevBuf table, lp;
    ohw_command_table host{};
    std::vector<int32_t> child_off, path, child_tok, terminal, phrase_id, src_tok, src_off;
    float penalty = OHW_COMMAND_PENALTY_DEFAULT;
    bool on = false;
  } cm;
  // kernel launches of the three device rules (ohw_dbg_counter "phrase_boost", "repeat_rule", "command_rule"): counted on the
  // host, so a captured step counts once, at its capture
  int64_t tally_phrase = 0, tally_repeat = 0, tally_command = 0;

  LogitRules() = default;
  LogitRules(const LogitRules&) = delete;
  LogitRules& operator=(const LogitRules&) = delete;
  void init(int device_, int n_vocab_, int eot_, int max_batch_, const hipStream_t* stream_) {
    device = device_; n_vocab = n_vocab_; eot = eot_; max_batch = max_batch_; stream = stream_;
  }

  // the bodies of ohw_state_set_logit_bias / _phrase_table / _repeat_rule / _command_table (include/ohw.h has the contracts)
  void set_bias(const float* values, int n);
  void set_phrases(const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases);
  void set_repeat(float penalty, int ngram);
  void set_commands(const int32_t* tokens, const int32_t* offsets, int n_phrases, float penalty);
  // the device half of the three setters: a prebuilt table, or the values, into the (lazily made) device buffers.  The test
  // entries use them on an instance of their own
  void upload_phrases(const ohw_phrase_table* t, int table_vocab);
  void upload_repeat(float penalty, int ngram);
  void upload_commands(const ohw_command_table* t, float penalty);

  // The device rules that are on, ahead of a sampler launch, in THE order: boost, repetition, commands (the bias is the
  // sampler's: bias_device).  kernels.hpp states the row mapping.  Null n_cur means every history is empty: the repetition rule
  // is skipped, the command list is not (the first step is where its root applies).  lp_group: the decoder rows per window among
  // the launch rows (0: group), which only list_logprob needs.  p gives n_vocab, max_tokens, eot and the token histories
  void apply(float* logits, int64_t ld, const SamplerParams& p, int rows, int row_mul, int group, const int32_t* n_cur, const int32_t* done,
             hipStream_t s, int lp_group = 0);
  // the same on the host for one row, and the bias behind it as the device samplers add it: what a host-sampled rung applies.
  // list_lp: written by the command list at a step whose history holds no text token.  Returns an OHW_* code (g_last_error set)
  int apply_host(const int32_t* history, int n, float* row, int n_vocab_, int eot_, float* list_lp) const;
  const float* bias_device() const { return bias.on ? bias.dev.as<float>() : nullptr; }

  // make this object's four rules equal src's: rule by rule through the setters, and only where the sources differ (arrays
  // bit by bit; counts, penalties and the n-gram size by value).  A rule that is off on both sides costs nothing
  void sync_from(const LogitRules& src);

  int phrase_count() const { return ph.on ? ph.host.n_phrases : 0; }
  int command_count() const { return cm.on ? cm.host.n_phrases : 0; }
  void list_logprob(int batch, float* out) const;
};

}  // namespace ohw
