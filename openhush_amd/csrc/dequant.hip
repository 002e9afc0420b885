// dequant.hip — ggml block-quantised tensors (dequant.hpp) -> fp32 staging, on the device (gfx950).
// The loader uploads a tensor's blocks as they are in the file and expands them here; the placer then sees the same
// fp32 staging buffer an f16 / f32 tensor gives it.
#include "dequant.hpp"
#include "kernels.hpp"

namespace ohw {

// Blocks are 18 / 20 / 22 / 24 / 34 bytes: 2-byte aligned only, so no lane may load "its" block as dwords.  A workgroup
// takes a chunk of DQ_CHUNK consecutive blocks instead: DQ_CHUNK * block bytes is a multiple of 4 for every type, so the
// chunk is a dword-aligned span that the lanes copy to LDS with coalesced dword loads; each lane then decodes output
// i, i + 256, ... from LDS (the 32 lanes of one block read the same d / m / qh: LDS broadcasts) and the stores of a wave
// are 256 contiguous bytes.
constexpr int DQ_CHUNK = 128;
constexpr int DQ_THREADS = 256;

template <int TT>
__global__ __launch_bounds__(DQ_THREADS) void dequant_blocks_kernel(const uint32_t* __restrict__ raw, float* __restrict__ dst, int64_t nblocks) {
  // d * q + m is two rounded operations (dequant.hpp): no mul+add contraction
#pragma clang fp contract(off)
  constexpr int BS = quant_block_bytes(TT);
  constexpr int CHUNK_DW = DQ_CHUNK * BS / 4;
  static_assert(BS > 0 && (DQ_CHUNK * BS) % 4 == 0, "a chunk must be a whole number of dwords");
  __shared__ uint32_t lds[CHUNK_DW];
  const unsigned char* lb = (const unsigned char*)lds;
  const uint16_t* lh = (const uint16_t*)lds;
  const int tid = threadIdx.x;
  const int64_t nchunks = (nblocks + DQ_CHUNK - 1) / DQ_CHUNK;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t b0 = ch * DQ_CHUNK;
    const int nb = nblocks - b0 < DQ_CHUNK ? (int)(nblocks - b0) : DQ_CHUNK;
    const int bytes = nb * BS;   // even; the last chunk may end on half a dword
    const uint32_t* src = raw + ch * CHUNK_DW;
    const int ndw = bytes >> 2;
    for (int i = tid; i < ndw; i += DQ_THREADS) lds[i] = src[i];
    if ((bytes & 2) && tid == 0) ((uint16_t*)lds)[2 * ndw] = ((const uint16_t*)src)[2 * ndw];
    __syncthreads();
    float* out = dst + b0 * QK;
    const int nout = nb * QK;
    for (int i = tid; i < nout; i += DQ_THREADS) {
      const int blk = i >> 5, j = i & 31, jl = j & 15;
      const int hb = blk * (BS / 2);   // the block's first half-word
      const unsigned char* p = lb + blk * BS;
      const float d = (float)__builtin_bit_cast(_Float16, lh[hb]);
      float y;
      if constexpr (TT == TT_Q8_0) {
        y = (float)(int)(signed char)p[2 + j] * d;
      } else if constexpr (TT == TT_Q4_0) {
        const int q = p[2 + jl];
        y = (float)((j < 16 ? q & 15 : q >> 4) - 8) * d;
      } else if constexpr (TT == TT_Q4_1) {
        const float m = (float)__builtin_bit_cast(_Float16, lh[hb + 1]);
        const int q = p[4 + jl];
        y = (float)(j < 16 ? q & 15 : q >> 4) * d + m;
      } else {
        constexpr int H = TT == TT_Q5_0 ? 1 : 2;   // half-words before qh
        const uint32_t qh = (uint32_t)lh[hb + H] | ((uint32_t)lh[hb + H + 1] << 16);
        const int q = p[2 * H + 4 + jl];
        const int x = j < 16 ? (q & 15) | (int)(((qh >> jl) << 4) & 16) : (q >> 4) | (int)((qh >> (jl + 12)) & 16);
        if constexpr (TT == TT_Q5_0) {
          y = (float)(x - 16) * d;
        } else {
          const float m = (float)__builtin_bit_cast(_Float16, lh[hb + 1]);
          y = (float)x * d + m;
        }
      }
      out[i] = y;
    }
    __syncthreads();
  }
}

template <int TT>
static void launch_typed(const void* raw, float* dst, int64_t nblocks, hipStream_t s) {
  const int64_t nchunks = (nblocks + DQ_CHUNK - 1) / DQ_CHUNK;
  const int blocks = (int)(nchunks < 8192 ? nchunks : 8192);
  hipLaunchKernelGGL((dequant_blocks_kernel<TT>), dim3(blocks), dim3(DQ_THREADS), 0, s, (const uint32_t*)raw, dst, nblocks);
  HIP_CHECK(hipGetLastError());
}

void launch_dequant_blocks(int ttype, const void* raw, float* dst, int64_t n, hipStream_t s) {
  if (n <= 0 || n % QK != 0) throw Error(OHW_E_INVALID_ARG, "dequantize: the element count must be a positive multiple of 32");
  if (((uintptr_t)raw & 3) != 0) throw Error(OHW_E_INVALID_ARG, "dequantize: the block buffer must be 4-byte aligned");
  const int64_t nblocks = n / QK;
  switch (ttype) {
    case TT_Q4_0: launch_typed<TT_Q4_0>(raw, dst, nblocks, s); break;
    case TT_Q4_1: launch_typed<TT_Q4_1>(raw, dst, nblocks, s); break;
    case TT_Q5_0: launch_typed<TT_Q5_0>(raw, dst, nblocks, s); break;
    case TT_Q5_1: launch_typed<TT_Q5_1>(raw, dst, nblocks, s); break;
    case TT_Q8_0: launch_typed<TT_Q8_0>(raw, dst, nblocks, s); break;
    default: throw Error(OHW_E_INVALID_ARG, "dequantize: ttype must be 2 (Q4_0), 3 (Q4_1), 6 (Q5_0), 7 (Q5_1) or 8 (Q8_0)");
  }
}

}  // namespace ohw
