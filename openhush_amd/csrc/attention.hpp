// attention.hpp — encoder self-attention (flash-style, non-causal, d_head = 64), gfx950.
#pragma once
#include "common.hpp"

namespace ohw {
// qkv: T [B*T][3*d] (q | k | v, head h at columns h*64), out: T [B*T][d]
// win_len (device i32 [batch], or null): per-window contexts - window b attends over its first win_len[b] rows, the row stride
// per window stays t_len; rows of query blocks wholly past win_len[b] are written as zeros, the other rows past it are unspecified
template <typename T> void launch_encoder_attention(const void* qkv, void* out, int batch, int t_len, int n_head, hipStream_t stream,
                                                    const int32_t* win_len = nullptr);
}  // namespace ohw
