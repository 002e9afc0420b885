// tokenize.cpp — text -> token ids for prompts (ohw_tokenize*), and the prompt clipping rule.  Host only.
//
// The scheme is whisper.cpp's, restated from memory (unpinned, no reference source was at hand): the text is
// split into pieces, and inside a piece the longest vocabulary entry that is a prefix of the rest is taken, again and again.
// Pieces, tried in this order at every position, each as long as it can be:
//   1. a contraction: ' followed by s, t, re, ve, m, ll or d
//   2. an optional space (0x20), then a run of letters: A-Z, a-z and every byte >= 0x80 (UTF-8 lead and continuation bytes)
//   3. an optional space, then a run of digits 0-9
//   4. an optional space, then a run of bytes that are neither white space, letters nor digits
//   5. a run of white space (0x20, \t, \n, \v, \f, \r)
// A byte that no entry starts with is skipped.  Of equal entries the lowest id wins; empty entries never match.
#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "model.hpp"

namespace ohw {
extern thread_local std::string g_last_error;
}

namespace {

bool is_letter(unsigned char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c >= 0x80; }
bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
bool is_space(unsigned char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
bool is_other(unsigned char c) { return !is_letter(c) && !is_digit(c) && !is_space(c); }

// length of the piece that starts at s[i] (n bytes in all, i < n): at least 1
size_t piece_len(const unsigned char* s, size_t i, size_t n) {
  if (s[i] == '\'' && i + 1 < n) {
    static const char* const tails[] = {"s", "t", "re", "ve", "m", "ll", "d"};
    for (const char* t : tails) {
      const size_t k = std::char_traits<char>::length(t);
      if (i + 1 + k <= n && std::equal(t, t + k, (const char*)s + i + 1)) return 1 + k;
    }
  }
  const size_t j = i + (s[i] == ' ' && i + 1 < n ? 1 : 0);      // behind the optional space
  bool (*const kinds[])(unsigned char) = {is_letter, is_digit, is_other};
  for (auto kind : kinds) {
    if (!kind(s[j])) continue;
    size_t e = j;
    while (e < n && kind(s[e])) ++e;
    return e - i;
  }
  size_t e = i;
  while (e < n && is_space(s[e])) ++e;
  return e - i;      // s[i] is white space here: every other byte is a letter, a digit or "other"
}

struct Vocab {
  std::unordered_map<std::string, int32_t> id;
  size_t longest = 0;
  void add(const char* p, size_t len, int32_t i) {
    if (len == 0) return;
    id.emplace(std::string(p, len), i);       // the first (lowest) id of equal entries stays
    longest = std::max(longest, len);
  }
};

// the number of tokens of text; the first cap of them are written
int64_t tokenize(const Vocab& v, const char* text, int32_t* out, int64_t cap) {
  const unsigned char* s = (const unsigned char*)text;
  const size_t n = std::char_traits<char>::length(text);
  int64_t count = 0;
  std::string key;
  for (size_t i = 0; i < n;) {
    const size_t end = i + piece_len(s, i, n);
    while (i < end) {
      size_t len = std::min(v.longest, end - i);
      for (; len > 0; --len) {
        key.assign(text + i, len);
        const auto it = v.id.find(key);
        if (it == v.id.end()) continue;
        if (count < cap) out[count] = it->second;
        ++count;
        break;
      }
      i += len > 0 ? len : 1;       // no entry starts here: the byte is skipped
    }
  }
  return count;
}

int finish(int64_t count, int cap, const char* what) {
  if (count > cap) {
    ohw::g_last_error = std::string(what) + ": the text has " + std::to_string(count) + " tokens, the buffer holds " + std::to_string(cap);
    return OHW_E_INVALID_ARG;
  }
  return (int)count;
}

}  // namespace

extern "C" {

int ohw_tokenize_host(const char* vocab_bytes, const int32_t* lens, int n_vocab, const char* text, int32_t* out, int cap) {
  if (n_vocab < 0 || (n_vocab > 0 && (!vocab_bytes || !lens)) || !text || cap < 0 || (cap > 0 && !out)) {
    ohw::g_last_error = "tokenize_host: bad argument";
    return OHW_E_INVALID_ARG;
  }
  Vocab v;
  size_t off = 0;
  for (int i = 0; i < n_vocab; ++i) {
    if (lens[i] < 0) {
      ohw::g_last_error = "tokenize_host: entry " + std::to_string(i) + " has a negative length";
      return OHW_E_INVALID_ARG;
    }
    v.add(vocab_bytes + off, (size_t)lens[i], i);
    off += (size_t)lens[i];
  }
  return finish(tokenize(v, text, out, cap), cap, "tokenize_host");
}

int ohw_tokenize(const ohw_ctx* ctx, const char* text, int32_t* out, int cap) {
  if (!ctx || !text || cap < 0 || (cap > 0 && !out)) {
    ohw::g_last_error = "tokenize: bad argument";
    return OHW_E_INVALID_ARG;
  }
  Vocab v;      // text tokens only: ids below end-of-text
  const size_t n = std::min(ctx->vocab.size(), (size_t)std::max(0, ctx->tok.eot));
  for (size_t i = 0; i < n; ++i) v.add(ctx->vocab[i].data(), ctx->vocab[i].size(), (int32_t)i);
  return finish(tokenize(v, text, out, cap), cap, "tokenize");
}

int ohw_prompt_clip_host(const int32_t* in, int n, int n_text_ctx, int32_t* out) {
  if (n < 0 || (n > 0 && (!in || !out)) || n_text_ctx < 2) {
    ohw::g_last_error = "prompt_clip_host: bad argument";
    return OHW_E_INVALID_ARG;
  }
  const int keep = std::min(n, n_text_ctx / 2 - 1);      // the LAST n_text_ctx / 2 - 1 tokens
  std::copy(in + (n - keep), in + n, out);
  return keep;
}

}  // extern "C"
