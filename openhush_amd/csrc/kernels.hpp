// kernels.hpp — launchers of the non-GEMM kernels of the hot path (gfx950).
#pragma once
#include <vector>

#include "common.hpp"

namespace ohw {

// ---- weights (weights.hip) ---------------------------------------------------------------------
// dst[i] = value of the procedural generator (openhush_amd/synth.py) for flat index i
void launch_synth_fill(float* dst, int64_t n, uint32_t key, float scale, float offset, int round_f16, hipStream_t s);
void launch_f16_to_f32(const void* src_f16, float* dst, int64_t n, hipStream_t s);
// ggml block-quantised tensor (dequant.hpp: ttype 2 Q4_0, 3 Q4_1, 6 Q5_0, 7 Q5_1, 8 Q8_0) -> f32; raw: n / 32 blocks as
// stored in the file, 4-byte aligned; throws OHW_E_INVALID_ARG for another ttype or n % 32 != 0 (dequant.hip)
void launch_dequant_blocks(int ttype, const void* raw_blocks, float* dst, int64_t n, hipStream_t s);
// plain row-major convert: dst T [rows][cols] (dst row stride ld_dst) from src f32 [rows][cols]
template <typename T> void launch_convert_rows(const float* src, void* dst, int64_t rows, int64_t cols, int64_t ld_dst, hipStream_t s);
// conv weight [d_out][c_in][3] f32 -> T [d_out][3][c_pad]
template <typename T> void launch_repack_conv(const float* src, void* dst, int64_t d_out, int64_t c_in, int64_t c_pad, hipStream_t s);
// decoder linear [N][K] f32 -> MFMA-fragment tiles T [Npad/16][K/32][64][8], rows >= N zero
template <typename T> void launch_repack_tiled(const float* src, void* dst, int64_t N, int64_t n_pad, int64_t K, hipStream_t s);
// wsum[n] = sum_k of the rounded 16-bit values of a fragment-tiled [N][K] matrix
template <typename T> void launch_tiled_rowsum(const void* w_tiled, float* wsum, int64_t N, int64_t K, hipStream_t s);
// fold a pre-LayerNorm's affine part into the linear layer that follows it (in place, f32 [N][K]):
//   bias[n] += sum_k beta[k] * W[n][k];  W[n][k] *= gamma[k]      so that  LN(x) W^T + b == ((x - mean) rstd) W'^T + b'
void launch_fold_ln(float* w, float* bias, const float* gamma, const float* beta, int64_t N, int64_t K, hipStream_t s);

// ---- front end (mel.hip) -----------------------------------------------------------------------
struct MelParams {
  const float* pcm;         // device [batch][pcm_stride]
  int64_t pcm_stride;
  const int32_t* n_samples; // device [batch]
  const float* filters;     // device [n_mels][201]
  const float* twiddle;     // device [2][400]: cos, sin of 2*pi*i/400
  const float* window;      // device [400] periodic Hann
  float* logmel;            // device [batch][n_mels][3000] (log10 power, then normalised in place)
  int32_t* max_bits;        // device [batch] ordered-int running max
  void* mel_t;              // device T [batch][3002][128] time-major image for conv1
  int32_t n_mels, batch, mode;
  // windows of a whole recording's spectrogram (ohw_recording_set / ohw_mel_seek): pcm is the recording (n_total samples),
  // window b starts at sample offsets[b] of it - real neighbouring samples at its edges, the reflection only at the
  // recording's start, zeros after its end; shared_max: ONE running maximum, max_bits[0], for all windows;
  // max_only: no spectrogram is stored (the pass that finds the recording's maximum)
  const int64_t* offsets = nullptr;
  int64_t n_total = 0;
  int32_t shared_max = 0, max_only = 0;
  // recording slots (ohw_recording_set_slot / ohw_mel_seek_slots): small device tables [batch]; window b reads the recording
  // win_pcm[b] of win_len[b] samples at offsets[b] and is clamped with max_bits[win_max[b]] (each slot's own maximum); null:
  // the one recording above (pcm, n_total, max_bits[0])
  const float* const* win_pcm = nullptr;
  const int64_t* win_len = nullptr;
  const int32_t* win_max = nullptr;
  // reduced audio context: frames >= frame_limit go into the time-major image as zeros, the conv padding value (the fp32
  // log-mel output is untouched); 0 = all 3000 frames
  int32_t frame_limit = 0;
  // per-window contexts (device i32 [batch], or null): window b's limit is 2 * win_ctx[b] instead of frame_limit
  const int32_t* win_ctx = nullptr;
};
template <typename T> void launch_mel(const MelParams& p, hipStream_t s);

// ---- normalisation (misc.hip) --------------------------------------------------------------------
// tiled = true writes y in the decoder GEMMs' activation order (act_tiled_offset, common.hpp) instead of row-major
template <typename T> void launch_layernorm(const float* x, const float* gamma, const float* beta, void* y, int64_t rows, int d, hipStream_t s,
                                            bool tiled = false);
template <typename T> void launch_to_f32(const void* src, float* dst, int64_t n, hipStream_t s);
// packed-row encoder: off i32 [batch + 1] = exclusive prefix sum of win_len (device i32 [batch], each clamped to 0 .. t_len),
// row_map i32 [off[batch]]: packed row off[b] + t -> unpacked row b * t_len + t
void launch_pack_map(const int32_t* win_len, int batch, int t_len, int32_t* off, int32_t* row_map, hipStream_t s);
// dst f32 [rows][d] = the rows row_map[r] of src f32 [..][d]; src and dst must not overlap
void launch_pack_rows(const float* src, const int32_t* row_map, float* dst, int64_t rows, int d, hipStream_t s);

// ---- decoder step (decode.hip) ---------------------------------------------------------------------
enum DecEpilogue {
  DEPI_QKV = 0,        // n < d: q T [M][d]; d <= n < 2d: self-K cache; 2d <= n: self-V cache (+bias)
  DEPI_BIAS_T = 1,     // out T [M][N]
  DEPI_BIAS_GELU_T = 2, // out T in activation-tile order (it feeds mlp.2)
  DEPI_BIAS_RESID = 3, // x f32 [M][N] += v + bias
  DEPI_LOGITS = 4      // logits f32 [batch][ld_logits], only rows m with (m % n_new) == n_new - 1 (and all rows to out_all, if set)
};
struct DecGemmParams {
  const void* x;       // T activation tiles [ceil(M/16)][K/32][64][8] (act_tiled_offset); with ln != 0: f32 [M][K] residual stream, (x - mean) * rstd fused into the prologue
  int32_t ln;          //   (gamma / beta of that LayerNorm are folded into w / bias at load: launch_fold_ln)
  const void* w;       // tiled T [Npad/16][K/32][64][8]
  const float* bias;   // [N] or nullptr
  void* out;           // see DecEpilogue
  int32_t M, N, K, n_new;
  // DEPI_QKV
  void* k_cache; void* v_cache;     // T [B][H][n_text_ctx][64] of this layer
  const int32_t* n_past;            // device [B]
  int32_t d_model, n_head, n_ctx;
  int64_t ld_out;
  int32_t cu_budget;                // compute units the launch may use (0 = the whole device); picks n-tiles per workgroup
  // DEPI_BIAS_RESID with ksplit > 1: K is split over ksplit workgroups per output tile (see decode.hip)
  int32_t ksplit;                   // 0 / 1 = off
  int32_t slab_bytes;
  float* slab;                      // f32 [tiles][ksplit][512]
  unsigned* ticket;                 // [tiles], zero between launches (the kernel re-arms it)
  // post-norm path (ln == 0, pn != 0): x is the 16-bit tiled copy of the residual stream and the LayerNorm is applied AFTER
  // the product: out = rstd[m] * (x W^T - mean[m] * wsum[n]) + bias[n], mean / rstd from the per-16-column statistics the
  // producers of the residual stream publish (no full-row read, no LayerNorm prologue, no LDS image)
  int32_t pn;
  int32_t n_stat;                   // statistics tiles per row (d_model / 16)
  const float* stat_in;             // f32 [M][n_stat][2]: mean and sum of squared deviations of 16 columns
  const float* wsum;                // f32 [N]
  // DEPI_BIAS_RESID producers: besides x (f32) also its 16-bit tiled copy and this tile's statistics (all null: off)
  void* x16_out;                    // T tiles [ceil(M/16)][N/32][64][8]
  float* stat_out;                  // f32 [M][N/16][2]
  // DEPI_QKV, single-token steps of at most 16 rows (attn_ticket != null): the masked self-attention of a head runs INSIDE this
  // launch, in the workgroup that publishes the last of the head's q / k / v columns (decode.hip) - no self-attention launch
  unsigned* attn_ticket;            // [n_head], zero between launches (the kernel re-arms it)
  void* attn_out;                   // T activation tiles [1][d_model/32][64][8]: what launch_self_attn would have written
  const int32_t* attn_slots;        // beam search: i32 [rows][n_ctx] (launch_self_attn's kv_slot), else null
  int64_t kv_bytes;                 // bytes of one layer's K (or V) cache: bound of the kernel's buffer descriptors
  // ln != 0, QKV and BIAS_GELU_T: scratch of the all-rows forms, T tiles [ceil(M/16)][K/32][64][8] - the LayerNorm of the rows,
  // written by a launch of its own in front of the GEMM (decode.hip, dec_ln_rows_kernel); null: those forms are not picked
  void* ln_rows;
  // DEPI_LOGITS: besides out, every row m < M and column n < N also goes to out_all[m * ld_all + n] (ohw_state_score reads a
  // chunk's 8 rows per window).  null: off - the launch is what it is without this field; the shape choice never looks at it
  float* out_all;
  int64_t ld_all;
};
// the launchers below return which instantiation they launched (the state tallies them: ohw_dbg_counter); the pick itself
// does not depend on the tally
// n-tiles x m-tiles per workgroup; 4x6 / 5x6: the all-rows forms behind a LayerNorm launch (two passes of three m-tiles)
// widest K of the LN forms (fused LayerNorm: 16 threads per row, 20 float4 each).  The engine runs LN1 + QKV, the cross query
// and LN2 + mlp.0 through them at K = n_text_state on every decode, so this is also the widest model check_hparams (model.hip)
// lets load: one constant for both
constexpr int DG_LN_MAXK = 1280;
enum DecGemmShape { DG_SHAPE_1x1, DG_SHAPE_2x1, DG_SHAPE_1x2, DG_SHAPE_2x2, DG_SHAPE_4x2, DG_SHAPE_1x6, DG_SHAPE_4x6, DG_SHAPE_5x6, DG_N_SHAPES };
template <typename T> int launch_dec_gemm(const DecGemmParams& p, int epilogue, hipStream_t s);

// x f32 [M][d] = token_embedding[tok[m]] + pos_emb[n_past[m / n_new] + m % n_new]
// x16 / stat (may be null): the 16-bit tiled copy and the per-16-column statistics of the post-norm path
template <typename T> void launch_embed(const void* emb_tiled, const float* pos, const int32_t* tok, const int32_t* n_past,
                                        float* x, void* x16, float* stat, int M, int n_new, int d, hipStream_t s);
// causal self-attention of the new tokens against the cache.  q T [M][d] -> out T, activation-tile order
// kv_slot (beam search, else null): i32 [rows][n_ctx], the cache row that holds position j of a row's sequence
enum SelfAttnVariant { SA_PLAIN, SA_SLOTS };
template <typename T> int launch_self_attn(const void* q, const void* k_cache, const void* v_cache, const int32_t* n_past,
                                            void* out, int M, int n_new, int n_head, int n_ctx, hipStream_t s, const int32_t* kv_slot = nullptr);
// cross-attention: q T [M][d]; cross K/V head-major T [B][H][t_len][64] of this layer -> out T, activation-tile order
// partials / tickets (may be null): scratch for cutting the keys of a (row, head) over up to XA_MAX_SPLIT workgroups when
// M <= max_split_rows leaves most CUs idle: f32 [max_split_rows][n_head][XA_MAX_SPLIT][68], u32 [max_split_rows][n_head] (zero)
constexpr int XA_MAX_SPLIT = 8;
// PLAIN: cross_attn_kernel, one workgroup per (row, head); SPLIT: the same with the keys cut over gridDim.z > 1 workgroups;
// ROWS<n>: cross_attn_rows_kernel<n> for n new tokens per window; GROUP<k>: the same for k beams per window; GROUP_SPLIT: beams
// through the split cross_attn_kernel
enum XattnVariant { XA_PLAIN, XA_SPLIT, XA_ROWS2, XA_ROWS3, XA_ROWS4, XA_GROUP2, XA_GROUP3, XA_GROUP4, XA_GROUP5, XA_GROUP_SPLIT, XA_N_VARIANTS };
template <typename T> int launch_cross_attn(const void* q, const void* xk, const void* xv, void* out, int M, int n_new,
                                             int n_head, int t_len, float* partials, unsigned* tickets, int max_split_rows,
                                             const int32_t* done /* [B] or null: windows whose rows are skipped */, hipStream_t s,
                                             int kv_group = 1 /* beam search: consecutive rows that share one window's K/V */,
                                             bool batch_invariant = false /* pick the variant from n_new alone, never from M */,
                                             const int32_t* win_len = nullptr /* device [windows] or null: window w streams its first
                                                win_len[w] keys of a slab whose stride stays t_len; implies batch_invariant's variant choice */);
// the n_q (8 or 16) query rows per window of one prefill chunk (ohw_state_prefill): q T [windows * n_q][d], row b * n_q + i; one
// workgroup per (head, window) streams K/V once for the rows, both products on the MFMA units (cross_attn_chunk_kernel).  done /
// win_len as above
template <typename T> void launch_cross_attn_chunk(const void* q, const void* xk, const void* xv, void* out, int windows, int n_head, int t_len,
                                                   const int32_t* done, const int32_t* win_len, hipStream_t s, int n_q = 8);

// ---- the 32 decoder layers of a single-token step in ONE persistent launch, at most 16 rows (decode_persist.hip) ----------
struct PersistLayer {
  const void *wqkv, *wo, *wxq, *wxo, *w1, *w2;       // fragment tiles T [N/16][K/32][64][8]
  const float *bqkv, *bo, *bxq, *bxo, *b1, *b2;
};
struct PersistParams {
  const PersistLayer* layers;     // device [L]
  int32_t L, M, group, d, H, n_ctx, t_len, S, nsplit;   // rows, rows per window, d_model, heads, positions, encoder positions, cross key slices, mlp.2 K slices
  const int32_t* n_past;     // [M]
  const int32_t* kv_slot;    // [M][n_ctx] or null (beam search)
  const int32_t* done;       // [M / group] or null: windows whose cross-attention is skipped
  const float* x_in;         // f32 [M][d]: the embedding launch's output
  float* x_out;              // f32 [M][d]: what the final LayerNorm launch reads (may alias x_in)
  void* self_kv;             // T [L][2][rows][H][n_ctx][64]
  int64_t kv_layer, kv_row;  // elements per K (or V) cache of a layer; per cache row
  const void* xkv;           // T [2L][windows][H][t_len][64]
  int64_t xkv_slab;
  unsigned long long* g;     // ONE granule arena (8-byte {payload | tag}); the regions below are offsets into it
  int32_t o_x, o_q, o_kv, o_a, o_qx, o_h, o_xp, o_mp;
  unsigned* epoch;           // device word, 1 at first use; bumped by every completed launch
  unsigned* abort_word;      // device word, 0; phase + 1 when a workgroup gave up waiting
};
// granules a state's arena needs for up to 16 rows; fills the offsets of p
int64_t persist_layout(PersistParams* p);
template <typename T> void launch_persist_step(const PersistParams& p, int grid, hipStream_t s);

// device-side logits filter + arg-max (restates oracle ref_process_logits)
struct SamplerParams {
  const float* logits;   // [batch][ld]
  int64_t ld;
  int32_t* tokens;       // [batch][max_tokens] sampled so far
  int32_t* n_cur;        // [batch]
  int32_t* n_past;       // [batch]   (advanced by one for live windows)
  int32_t* next_tok;     // [batch]   token to feed next
  int32_t* done;         // [batch]
  int32_t* n_done;       // [1] number of finished windows
  float* sum_logprob;    // [batch]
  int32_t batch, max_tokens, n_vocab;
  int32_t eot, sot, translate, transcribe, solm, prev, nosp, no_ts, ts_begin, blank, n_langs;
  int32_t suppress_blank, no_timestamps, max_initial_ts, n_max, force_len, n_text_ctx;
  int32_t advance;       // 1: n_past[b] += 1 first (a single-token step ran since the last call)
  // the row is scanned by SAMPLER_SPLIT workgroups per window; the one that draws the last ticket merges the partials
  float* partials;       // [batch][SAMPLER_SPLIT][SAMPLER_PART_WORDS]
  unsigned* tickets;     // [batch], zero between launches (re-armed by the kernel)
  const float* bias;     // [n_vocab] added to every logit before the filter, or null (ohw_state_set_logit_bias)
  float* tok_lp;         // [batch][max_tokens + 1] log-probability of every sampled token; the end-of-text token's goes
                         //   to slot n_cur without being counted (whisper.cpp sums it into avg_logprobs), or null
  float* nosp_prob;      // [batch] softmax probability of the no-speech token in the window's first, unfiltered row, or null
};
// beam search state of a batch of windows (decode.hip): beam j of window w is decoder row w * K + j
struct BeamParams {
  int32_t K;              // beam size, 2..5
  int32_t prefix_stride;  // first step: the shared past of window w (prompt pass, context) lives in cache row w * prefix_stride:
                          //   1, or K under a context table (ohw_beam_search moves it there: launch_kv_prefix_move)
  float* cand_lp;         // [rows][K + 1] log-probabilities of every row's best next tokens
  int32_t* cand_tok;      // [rows][K + 1]
  float* beam_sum;        // [rows] cumulative log-probability
  int32_t* kv_slot;       // [rows][n_text_ctx] self-K/V row per position (this step's view)
  int32_t* kv_slot_next;  // the other half of the double buffer (written by the update, read by the next step)
  int32_t* tokens_next;   // [rows][max_tokens] the other half of the token-history double buffer
  int32_t* n_cur;         // [windows] tokens sampled so far
  int32_t* n_past_w;      // [windows] position written by the step that just ran
  int32_t* win_done;      // [windows]
  int32_t* fin_cnt;       // [windows] finished sequences in the pool (at most K)
  int32_t* fin_tok;       // [windows][K][max_tokens]
  int32_t* fin_len;       // [windows][K]
  float* fin_sum;         // [windows][K] cumulative log-probability, the end-of-text token's included
  unsigned* part;         // [rows][BEAM_SPLIT][BEAM_PART_WORDS] slice states of the split top-k (beam_topk_kernel)
  unsigned* tickets;      // [rows], zero between launches (re-armed by the kernel)
  // what a decode policy needs of the result (ohw_beam_search_ex); null: the kernels touch none of it
  const float* plog;      // [rows][max_tokens + 1] log-probability of every token of a beam's history (this step's view), or null
  float* plog_next;       // the other half of the double buffer: gathered like tokens_next, the chosen candidate's own cand_lp at n_cur
  float* fin_plog;        // [windows][K][max_tokens + 1] the same for the pool; end-of-text's at index fin_len
  float* nosp_prob;       // [windows] first step: soft-max probability of the no-speech token in the unfiltered row, or null
};
constexpr int BEAM_SPLIT = 8;         // workgroups per logits row
constexpr int BEAM_PART_WORDS = 32;   // max, sum, timestamp sum, best text logit, then (K + 1) text and (K + 1) timestamp candidates (value, index);
                                      //   words 28 / 29: the unfiltered row's max and sum (first step with nosp_prob only)
void launch_beam_step(const SamplerParams& p, const BeamParams& bp, int n_windows, int first, hipStream_t s);
// the final ranking of a beam search, one workgroup per window (decode.hip): the pool's sequences, then the live beams by
// descending cumulative log-probability until there are K; the best cumulative log-probability per token wins (first maximum)
struct BeamFinishParams {
  int32_t K, stride, max_tokens;   // beams per window; row length of the token arrays (log-probability rows: stride + 1); clip
  const int32_t *fin_cnt, *fin_len, *fin_tok, *n_cur, *tokens;
  const float *fin_sum, *fin_plog, *beam_sum, *plog;
  int32_t *out_tok, *out_n, *out_eot, *out_nfin;   // [windows][stride], [windows] ...
  float *out_lp, *out_sum;                         // [windows][stride + 1], [windows]
};
void launch_beam_finish(const BeamFinishParams& f, int n_windows, hipStream_t s);
// the same rule on the host (no GPU): the arrays are host memory
void beam_finish_host(const BeamFinishParams& f, int n_windows);
// self K/V cache T [planes][max_batch][n_head][n_ctx][64] (planes = 2 * layers): positions 0 .. n_pos - 1 of cache row src are
// copied to row dst in every plane and head.  Beam search under a context table: window w's shared past goes from row w to row
// w * K, a row only w's own beams write - row w is also the own row of a beam of window w / K, which would write into a longer context
template <typename T> void launch_kv_prefix_move(void* self_kv, int planes, int max_batch, int n_head, int n_ctx, int src, int dst, int n_pos, hipStream_t s);
constexpr int SAMPLER_SPLIT = 8;
constexpr int SAMPLER_PART_WORDS = 12;
void launch_sampler(const SamplerParams& p, hipStream_t s);
// the same filter at a temperature, then one draw (the fallback ladder on the device): temperature [1] and
// uniforms [batch][p.max_tokens] (the canonical double of step n_cur of row b) are read from device memory
void launch_sampler_t(const SamplerParams& p, const float* temperature, const double* uniforms, hipStream_t s);
// the group form (best-of sampling: ohw_sample_pass_n): p.batch rows are `group` candidates per window, row r = candidate
// r % group of window r / group, each with its own history, draws, done flag and every other per-row entry of p.  A row's
// arithmetic is launch_sampler_t's (one kernel body, sampler_t_row).  p.advance == 0 is the step behind the prompt: row r reads
// the WINDOW's logits row r / group.  The row that finishes last in a window (a ticket on win_cnt, agent scope) sets win_done
struct SampGroup {
  int32_t group;          // candidates per window, 1..5
  int32_t* win_done;      // [windows]: what run_decoder_step and the cross-attention get
  unsigned* win_cnt;      // [windows]: finished rows; the caller zeroes it per pass (`group` for a window that starts done)
};
void launch_sampler_group(const SamplerParams& p, const SampGroup& g, const float* temperature, const double* uniforms, hipStream_t s);
// the layout of a group pass, built where it lives: for row r = w * group + j (one workgroup per row)
//   kv_slot[r][i] = i < shared[w] ? w * prefix_stride : r  for i < n_ctx;  n_past[r] = shared[w];
//   done[r] = !active[w];  and by the rows with j == 0:  win_done[w] = !active[w], win_cnt[w] = active[w] ? 0 : group
struct SampGroupInit {
  int32_t rows, group, n_ctx, prefix_stride;
  const int32_t* shared;  // [windows]: positions of the window's shared past (context + prompt)
  const int32_t* active;  // [windows]
  int32_t *kv_slot, *n_past, *done, *win_done;
  unsigned* win_cnt;
};
void launch_sample_group_init(const SampGroupInit& q, hipStream_t s);

// ---- hot phrases (phrase.hip; ohw_state_set_phrase_table) ---------------------------------------------------------------
// The trie of include/ohw.h's ohw_phrase_table in ONE device buffer of fixed size (the limits' worth), so the pointers a
// captured step bakes in hold for every table set later.  Offsets in 4-byte words:
constexpr int PH_MAX_NODES = 1 + OHW_PHRASE_MAX_PHRASES * (OHW_PHRASE_MAX_LEN - 1);
constexpr int PH_MAX_EDGES = OHW_PHRASE_MAX_PHRASES * OHW_PHRASE_MAX_LEN;
constexpr int PH_MAX_PATH = OHW_PHRASE_MAX_PHRASES * (OHW_PHRASE_MAX_LEN - 1) * OHW_PHRASE_MAX_LEN / 2;
constexpr int PH_OFF_DEPTH = 0;                                  // i32 [17] depth_start
constexpr int PH_OFF_BASE = 32;                                  // i32 [16] path_base
constexpr int PH_OFF_CHILD = 64;                                 // i32 [PH_MAX_NODES + 1] child_off
constexpr int PH_OFF_PATH = PH_OFF_CHILD + PH_MAX_NODES + 1;     // i32 [PH_MAX_PATH]
constexpr int PH_OFF_TOK = PH_OFF_PATH + PH_MAX_PATH;            // i32 [PH_MAX_EDGES] child_tok
constexpr int PH_OFF_BOOST = PH_OFF_TOK + PH_MAX_EDGES;          // f32 [PH_MAX_EDGES] child_boost
constexpr int PH_WORDS = PH_OFF_BOOST + PH_MAX_EDGES;
// launch row r (one workgroup each) boosts logits row r with the history of decoder row h = r * row_mul, whose length and
// done flag are those of entry h / group: n_cur[h / group] (null: every history is empty) and done[h / group].
//   greedy, temperature and group passes: row_mul = group = 1;  the group pass's first step: the windows' rows, n_cur null
//   beam search: group = K with the windows' n_cur and done flags; its first step: the windows' rows, row_mul = K
struct PhraseBoostParams {
  float* logits;            // [rows][ld], changed in place over columns [0, n_vocab)
  int64_t ld;
  int32_t n_vocab, max_tokens, row_mul, group;
  const int32_t* tokens;    // [decoder rows][max_tokens]; entries at and behind n_cur are never read
  const int32_t* n_cur;
  const int32_t* done;
  const int32_t* table;     // the PH_WORDS buffer
};
void launch_phrase_boost(const PhraseBoostParams& p, int rows, hipStream_t s);
// the two host twins (no device): the builder and the rule that include/ohw.h defines
void phrase_table_build_host(const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases, int eot, ohw_phrase_table* out);
void phrase_boost_host(const ohw_phrase_table* t, const int32_t* history, int n_cur, float* row, int n_vocab);
// the table's arrays laid out as the device buffer above (PH_WORDS words); checks every count and child token against n_vocab
void phrase_table_pack(const ohw_phrase_table* t, int n_vocab, std::vector<int32_t>* words);

// ---- repetition penalty and no-repeat n-grams (repeat.hip; ohw_state_set_repeat_rule) ------------------------------------
// PhraseBoostParams' twin: the same row mapping (launch row r changes logits row r with the history of decoder row
// h = r * row_mul, length n_cur[h / group] - null: every history is empty - and flag done[h / group]).  rule: two words the
// state owns, {the fp32 bits of the penalty, the n-gram size}; a captured step holds the pointer, so new values capture nothing.
struct RepeatRuleParams {
  float* logits;            // [rows][ld], changed in place over the columns of text tokens, [0, min(eot, n_vocab))
  int64_t ld;
  int32_t n_vocab, max_tokens, row_mul, group, eot;
  const int32_t* tokens;    // [decoder rows][max_tokens]; entries at and behind n_cur are never read
  const int32_t* n_cur;
  const int32_t* done;
  const int32_t* rule;
};
void launch_repeat_rule(const RepeatRuleParams& p, int rows, hipStream_t s);
// the values ohw_state_set_repeat_rule accepts (throws Error otherwise), and the rule on one row on the host (no device)
void repeat_rule_check(float penalty, int ngram);
void repeat_rule_host(float penalty, int ngram, const int32_t* history, int n_cur, float* row, int n_vocab, int eot);

// ---- command lists (command.hip; ohw_state_set_command_table) ------------------------------------------------------------
// The anchored trie of include/ohw.h's ohw_command_table in ONE device buffer of fixed size, the penalty's fp32 bits with it, so
// the pointer a captured step bakes in holds for every list and penalty set later.  Offsets in 4-byte words:
constexpr int CM_DEPTHS = OHW_PHRASE_MAX_LEN + 1;                // depths 0 .. 16: the full phrases are nodes too
constexpr int CM_MAX_NODES = OHW_COMMAND_MAX_NODES;
constexpr int CM_MAX_EDGES = OHW_COMMAND_MAX_EDGES;
constexpr int CM_MAX_PATH = OHW_COMMAND_MAX_PATH;
constexpr int CM_OFF_DEPTH = 0;                                  // i32 [18] depth_start
constexpr int CM_OFF_BASE = 32;                                  // i32 [17] path_base
constexpr int CM_OFF_PENALTY = 60;                               // f32 the penalty (+inf: OHW_REPEAT_BAN)
constexpr int CM_OFF_CHILD = 64;                                 // i32 [CM_MAX_NODES + 1] child_off
constexpr int CM_OFF_TERM = CM_OFF_CHILD + CM_MAX_NODES + 1;     // i32 [CM_MAX_NODES] terminal
constexpr int CM_OFF_PATH = CM_OFF_TERM + CM_MAX_NODES;          // i32 [CM_MAX_PATH]
constexpr int CM_OFF_TOK = CM_OFF_PATH + CM_MAX_PATH;            // i32 [CM_MAX_EDGES] child_tok
constexpr int CM_WORDS = CM_OFF_TOK + CM_MAX_EDGES;
constexpr int CM_MAX_VOCAB = 1 << 18;                            // the children's bit map lives in LDS: 32 KiB at most
// PhraseBoostParams' row mapping (launch row r changes logits row r with the history of decoder row h = r * row_mul, length
// n_cur[h / group] - null: every history is empty - and flag done[h / group]).  list_logprob: the row h with
// h % lp_group == 0 writes list_logprob[h / lp_group] at a step where its history holds no text token; lp_group is the
// decoder rows per window (the beams, or a group pass's candidates; 1 where the launch rows are the windows).
struct CommandRuleParams {
  float* logits;            // [rows][ld], changed in place over columns [0, min(eot + 1, n_vocab))
  int64_t ld;
  int32_t n_vocab, max_tokens, row_mul, group, lp_group, eot;
  const int32_t* tokens;    // [decoder rows][max_tokens]; entries at and behind n_cur are never read
  const int32_t* n_cur;
  const int32_t* done;
  const int32_t* table;     // the CM_WORDS buffer
  float* list_logprob;
};
void launch_command_rule(const CommandRuleParams& p, int rows, hipStream_t s);
// the host twins (no device): the penalty the setter accepts (throws Error otherwise), the builder, the rule on one row
// (list_logprob_out, if given, is written only when the history holds no text token), the exact match of a result
void command_penalty_check(float penalty);
void command_table_build_host(const int32_t* tokens, const int32_t* offsets, int n_phrases, int eot, ohw_command_table* out);
void command_rule_host(const ohw_command_table* t, float penalty, const int32_t* history, int n_cur, float* row, int n_vocab, int eot,
                       float* list_logprob_out);
int command_match_host(const ohw_command_table* t, const int32_t* tokens, int n);
// the table's arrays and the penalty laid out as the device buffer above (CM_WORDS words); checks every count and index
void command_table_pack(const ohw_command_table* t, float penalty, std::vector<int32_t>* words);

// ---- vad.hip: the spectral speech detector (include/ohw.h, ohw_state_vad_frames).  All pointers are device pointers ----
constexpr int VAD_BINS = 320;          // histogram bins of 0.5 dB from -100 dB
struct VadParams {
  const float* pcm;         // n samples
  int64_t n;
  int64_t n_frames;         // (n + 159) / 160
  const float* twiddle;     // the mel front end's [2][400] cos / sin
  const float* window;      //   and its periodic Hann window [400]
  float* energy;            // [n_frames] band energies in dB
  int32_t* hist;            // [VAD_BINS], zeroed by launch_vad_floor_prob
  float* floor_db;          // [1]
  float* prob;              // [n_frames]
  int32_t target;           // the cumulative count that defines the floor: ceilf(q * n_frames), 1 .. n_frames
  float margin_db, slope_db;
};
void launch_vad_band(const VadParams& p, hipStream_t s);
void launch_vad_floor_prob(const VadParams& p, hipStream_t s);
// the detector's parameters as ohw.h states them (throws Error), and the target count of the floor's quantile
void vad_detector_check(const ohw_vad_detector& d);
int32_t vad_floor_target(float q, int64_t n_frames);

// ---- per-window language (decode.hip; ohw_state_set_window_lang) -------------------------------------------------------
constexpr int32_t LANG_PENDING = -1;  // table entry that waits for a detection (OHW_LANG_DETECT)
// one workgroup per window whose table entry lang[b] is LANG_PENDING (the others are left alone): over the raw columns
// logits[b * ld + sot + 1 + i], i < n_langs (no bias, no filter), lang[b] = the arg-max, the lowest index on ties, and
// lang_prob[b][0 .. n_langs) = the fp32 soft-max over those columns only (n_langs <= 128: two columns per lane).  ohw_lang_pick_host (host_engine.cpp) defines the result
void launch_lang_pick(const float* logits, int64_t ld, int sot, int n_langs, int32_t* lang, float* lang_prob, int batch, hipStream_t s);
// step_tok[b][0 .. n_prompt) = {sot, then sot + 1 + lang[b] and task when multilingual, then no_ts when no_ts >= 0} for b < batch:
// the prompt rows of a decode under a language table, built where the table lives.  Returns n_prompt
int launch_prompt_fill(const int32_t* lang, int32_t* step_tok, int batch, int sot, int multilingual, int task, int no_ts, hipStream_t s);

// ---- word timestamps (align.hip; ohw_state_align) -----------------------------------------------------------------------
// the listed heads of ONE decoder layer: workgroup x of the tap serves head head[x] and writes slot slot[x] of the caller's list
struct AlignTapList { int32_t n; int16_t slot[OHW_ALIGN_MAX_HEADS]; int16_t head[OHW_ALIGN_MAX_HEADS]; };
struct AlignTapParams {
  const void* q;            // T [windows * rows][64 * n_head]: the layer's cross-attention queries of this chunk (st->dq)
  const void* xk;           // T [windows][n_head][t_len][64]: the layer's cross K
  int32_t n_head, t_len;
  int32_t rows, row0;       // query rows per window in this launch (1..8); their first row index in p
  int32_t row_cap;          // rows of p per (window, head): rows from row_cap on are not stored
  int32_t lds_stride;       // >= every window's n_keys (more keys than that are not read), <= t_len
  const int32_t* n_keys;    // device [windows]: soft-max over keys 0 .. n_keys - 1
  const int32_t* n_all;     // device [windows] or null: rows from n_all[b] on are not stored
  float* p;                 // f32: p[b * p_win + a * p_head + row * p_row + t]
  int64_t p_win, p_head, p_row;
  int32_t p_fill;           // keys n_keys .. p_fill - 1 of a stored row are written as 0; p_fill <= p_row
  float* q_out;             // f32 [windows][row_cap][n_slots][64] or null: the rows as the logits use them (q * 0.125)
  int32_t n_slots;
};
template <typename T> void launch_align_tap(const AlignTapParams& p, const AlignTapList& list, int windows, hipStream_t s);
struct AlignReduceParams {
  const float* p;           // as AlignTapParams::p
  int64_t p_win, p_head, p_row;
  float* stats;             // f32 scratch [windows][n_heads][ld_stat][2]: mean and standard deviation of every key column
  int64_t ld_stat;
  int32_t n_heads, n_prompt;
  int32_t max_rows, max_keys;   // bounds of m: a window's n_all - n_prompt and n_keys are clamped to them
  const int32_t* n_all;     // device [windows]: token rows of the window (0: the window is skipped)
  const int32_t* n_keys;    // device [windows]
  float* m;                 // f32: m[b * m_win + k * m_row + t], k < n_all[b] - n_prompt
  int64_t m_win, m_row;
};
void launch_align_reduce(const AlignReduceParams& p, int windows, hipStream_t s);
struct AlignDtwParams {
  const float* m;           // as AlignReduceParams::m
  int64_t m_win, m_row;
  const int32_t* n_rows;    // device [windows]: rows of m (0: the window is skipped), clamped to max_rows
  const int32_t* n_keys;    // device [windows], clamped to max_keys
  uint8_t* trace;           // scratch [windows][trace_win], trace_win >= (max_rows + 1) * (max_keys + 1)
  int64_t trace_win;
  int32_t* idx;             // i32 [windows][idx_win]: the first key of every row, idx_win >= max_rows
  int64_t idx_win;
  int32_t max_rows, max_keys;
};
void launch_align_dtw(const AlignDtwParams& p, int windows, hipStream_t s);
// the host twins (no device): what the two launches above compute, bit for bit
void align_reduce_host(const float* p, int n_heads, int n_all, int n_prompt, int n_keys, float* m_out);
void dtw_host(const float* m, int n, int n_keys, int32_t* start_idx_out);

// ---- confidence (score.hip; ohw_state_score) ------------------------------------------------------------------------------
// One workgroup per logits row of a replay chunk: row m = b * 8 + j is position row0 + j of window b.  It writes entry
// row0 + j - (n_prompt - 1) of window b iff n_prompt - 1 <= row0 + j < n_all[b] (and the entry is below cap); every other row
// is neither read nor written.  The work shape is fixed by n_vocab alone (score.hip states the reduction order)
struct TokenScoreParams {
  const float* logits;      // f32 [batch * 8][ld], raw; columns n_vocab .. ld - 1 are padding and reach no result
  int64_t ld;               // ld % 4 == 0, 16-byte aligned rows
  const int32_t* targets;   // i32 [batch * 8]: the column whose logit row m reports
  const int32_t* n_all;     // i32 [batch]: positions of window b that have a score (0: the window is skipped)
  int32_t row0, n_prompt, n_vocab, eot, batch, cap;
  ohw_token_score* out;     // [batch][cap]
};
void launch_token_score(const TokenScoreParams& p, hipStream_t s);
// the rule on one row on the host (no device): the same fp32 operations in the kernel's order
void token_score_host(const float* x, int n_vocab, int eot, int target, ohw_token_score* out);

}  // namespace ohw
