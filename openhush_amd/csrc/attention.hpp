// attention.hpp — encoder self-attention (flash-style, non-causal, d_head = 64), gfx950.
#pragma once
#include "common.hpp"

namespace ohw {
// qkv: T [B*T][3*d] (q | k | v, head h at columns h*64), out: T [B*T][d]
// win_len (device i32 [batch], or null): per-window contexts - window b attends over its first win_len[b] rows, the row stride
// per window stays t_len; rows of query blocks wholly past win_len[b] are written as zeros, the other rows past it are unspecified
// win_off (device i32 [batch], needs win_len; or null): packed rows - window b's rows start at row win_off[b] of qkv and out (the
// exclusive prefix sum of win_len) instead of b * t_len; rows that are not window b's are never stored (they are a neighbour's)
template <typename T> void launch_encoder_attention(const void* qkv, void* out, int batch, int t_len, int n_head, hipStream_t stream,
                                                    const int32_t* win_len = nullptr, const int32_t* win_off = nullptr);
}  // namespace ohw
