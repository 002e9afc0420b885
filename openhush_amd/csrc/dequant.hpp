// dequant.hpp — ggml block-quantised tensor types the loader expands at load (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0).
// One block holds 32 consecutive values of the tensor's fastest dimension.  Layouts (little-endian, d / m IEEE f16):
//   Q4_0 18 B {d; u8 qs[16]}           Q4_1 20 B {d; m; u8 qs[16]}
//   Q5_0 22 B {d; u32 qh; u8 qs[16]}   Q5_1 24 B {d; m; u32 qh; u8 qs[16]}      Q8_0 34 B {d; i8 qs[32]}
// With j = 0 .. 15 (Q8_0: j = 0 .. 31), everything in fp32 after widening d and m, one rounding per operation:
//   Q4_0  y[j] = ((qs[j] & 15) - 8) * d          y[j+16] = ((qs[j] >> 4) - 8) * d
//   Q4_1  y[j] = (qs[j] & 15) * d + m            y[j+16] = (qs[j] >> 4) * d + m
//   Q5_0  x0 = (qs[j] & 15) | (((qh >> j) << 4) & 16), x1 = (qs[j] >> 4) | ((qh >> (j + 12)) & 16)
//         y[j] = (x0 - 16) * d                   y[j+16] = (x1 - 16) * d
//   Q5_1  y[j] = x0 * d + m                      y[j+16] = x1 * d + m
//   Q8_0  y[j] = qs[j] * d
// The kernel (dequant.hip) and the host twin (dequant_host.cpp) each restate these; tests hold them equal bit for bit.
#pragma once
#include <cstdint>

namespace ohw {

enum { TT_F32 = 0, TT_F16 = 1, TT_Q4_0 = 2, TT_Q4_1 = 3, TT_Q5_0 = 6, TT_Q5_1 = 7, TT_Q8_0 = 8 };
constexpr int QK = 32;   // values per block

// bytes of one block; 0 for a type that is not block-quantised (or not supported)
constexpr int quant_block_bytes(int ttype) {
  return ttype == TT_Q4_0 ? 18 : ttype == TT_Q4_1 ? 20 : ttype == TT_Q5_0 ? 22 : ttype == TT_Q5_1 ? 24 : ttype == TT_Q8_0 ? 34 : 0;
}

}  // namespace ohw
