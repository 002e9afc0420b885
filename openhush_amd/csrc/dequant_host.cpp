// dequant_host.cpp — host twin of dequant.hip: the ggml block formulas (dequant.hpp) restated in plain C++, no device
// needed.  CPU tests pin it against literal values and the numpy restatement; the GPU test holds the kernel equal to it.
#include <cstring>

#include "../../include/ohw.h"
#include "dequant.hpp"

namespace {

// IEEE f16 bits -> f32, exact (subnormals, infinities and NaN payloads included)
float half_to_float(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t exp = (h >> 10) & 31u, man = h & 0x3FFu, bits;
  if (exp == 31) {
    bits = sign | 0x7F800000u | (man << 13);
  } else if (exp != 0) {
    bits = sign | ((exp + 112) << 23) | (man << 13);
  } else if (man == 0) {
    bits = sign;
  } else {
    int e = 113;
    while (!(man & 0x400u)) { man <<= 1; --e; }
    bits = sign | ((uint32_t)e << 23) | ((man & 0x3FFu) << 13);
  }
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}
uint16_t rd16(const unsigned char* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
uint32_t rd32(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

}  // namespace

extern "C" int ohw_dequantize_host(int ttype, const void* blocks, int64_t n, float* out) {
#pragma clang fp contract(off)
  using namespace ohw;
  const int bs = quant_block_bytes(ttype);
  if (bs == 0 || !blocks || !out || n <= 0 || n % QK != 0) return OHW_E_INVALID_ARG;
  const unsigned char* p = (const unsigned char*)blocks;
  for (int64_t b = 0; b < n / QK; ++b, p += bs, out += QK) {
    const float d = half_to_float(rd16(p));
    if (ttype == TT_Q8_0) {
      for (int j = 0; j < 32; ++j) out[j] = (float)(int)(signed char)p[2 + j] * d;
    } else if (ttype == TT_Q4_0) {
      for (int j = 0; j < 16; ++j) {
        out[j] = (float)((p[2 + j] & 15) - 8) * d;
        out[j + 16] = (float)((p[2 + j] >> 4) - 8) * d;
      }
    } else if (ttype == TT_Q4_1) {
      const float m = half_to_float(rd16(p + 2));
      for (int j = 0; j < 16; ++j) {
        const float lo = (float)(p[4 + j] & 15) * d, hi = (float)(p[4 + j] >> 4) * d;
        out[j] = lo + m;
        out[j + 16] = hi + m;
      }
    } else {
      const int h = ttype == TT_Q5_0 ? 2 : 4;   // bytes before qh
      const float m = ttype == TT_Q5_1 ? half_to_float(rd16(p + 2)) : 0.0f;
      const uint32_t qh = rd32(p + h);
      const unsigned char* qs = p + h + 4;
      for (int j = 0; j < 16; ++j) {
        const int x0 = (qs[j] & 15) | (int)(((qh >> j) << 4) & 16);
        const int x1 = (qs[j] >> 4) | (int)((qh >> (j + 12)) & 16);
        if (ttype == TT_Q5_0) {
          out[j] = (float)(x0 - 16) * d;
          out[j + 16] = (float)(x1 - 16) * d;
        } else {
          const float lo = (float)x0 * d, hi = (float)x1 * d;
          out[j] = lo + m;
          out[j + 16] = hi + m;
        }
      }
    }
  }
  return OHW_OK;
}
