// gemm_small.hip — 64x64x64 LDS-tiled MFMA GEMM for the encoder of a SHORT window (gfx950).
//
// Under a reduced audio context (ohw_state_set_audio_ctx) one window is a few hundred rows: at M = 256 and large-v3 dims
// the 128x128 tiles of gemm.hip are 20 (attn.out, mlp.2), 60 (QKV) or 80 (mlp.0) workgroups on 256 compute units.  This
// kernel cuts the same problem into 64x64 tiles - four times the workgroups - and is otherwise gemm.hip's scheme:
//   C[M][N] = A[M][K] * W[N][K]^T, 16-bit operands, fp32 accumulate, v_mfma_f32_16x16x32 with SWAPPED operands (the weight
//   tile is the MFMA "A" operand), the n-rows of the weight tile permuted at staging time so a lane ends up with 16
//   contiguous output columns of ONE row (gemm_epilogue.hpp, every epilogue of gemm.hip);
//   256 threads = 4 waves, each wave 16 rows x 64 columns (1x4 MFMA tiles, 16 accumulator VGPRs) - all four read the whole
//   weight tile from LDS, which is the price of the small tile: 5 ds_read_b128 per 4 MFMAs against 8 per 16;
//   LDS: 2 stages x (64x64 A + 64x64 W) x 2 B = 32 KiB, 16-byte chunks XOR-swizzled by (row & 7); global -> LDS through
//   registers, the loads of K-step k+1 issued before the MFMAs of step k: one barrier per K-step.
// Every output element is accumulated over K in the order gemm.hip uses (32 columns per MFMA, ascending), so the two
// kernels give the same bits: which of them runs is a matter of speed only.
// Selected only through GemmParams::small_m (engine.hip, run_encode); ohw_dbg_gemm_small for the tests.
#include "gemm.hpp"
#include "gemm_epilogue.hpp"

namespace ohw {

constexpr int SM_BM = 64, SM_BN = 64, SM_BK = 64;
constexpr int SM_THREADS = 256;
constexpr int SM_STAGE = 16384;   // A tile 8 KiB | W tile 8 KiB

template <typename T, int EPI>
__global__ __launch_bounds__(SM_THREADS, 4) void gemm_small_kernel(GemmParams p) {
  using Ops = TypeOps<T>;
  using vec8 = typename Ops::vec8;
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * SM_STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  const unsigned n_tiles_n = (unsigned)(p.N / SM_BN);
  const unsigned n_tiles_m = (unsigned)((p.M + SM_BM - 1) / SM_BM);
  const unsigned nwg = n_tiles_n * n_tiles_m;
  const unsigned lid = xcd_remap(blockIdx.x, nwg);
  const int64_t m0 = (int64_t)(lid / n_tiles_n) * SM_BM;
  const int64_t n0 = (int64_t)(lid % n_tiles_n) * SM_BN;

  const T* __restrict__ A = (const T*)p.A;
  const T* __restrict__ W = (const T*)p.W;

  // ---- staging assignment: thread -> 2 rows x one 16-byte chunk, for each operand ----
  const int srow = tid >> 3;  // 0..31 (+32*i)
  const int chunk = tid & 7;
  const T* a_ptr[2];
  const T* w_ptr[2];
  int a_lds[2], w_lds[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = srow + 32 * i;
    int64_t m = m0 + r;
    if (m > p.M - 1) m = p.M - 1;          // clamped row: unconditional loads, masked stores
    int64_t b = 0, rr = m;
    if (p.rows_per_batch < p.M) { const unsigned bb = (unsigned)m / (unsigned)p.rows_per_batch; b = bb; rr = m - (int64_t)bb * p.rows_per_batch; }
    a_ptr[i] = A + b * p.a_batch_stride + rr * p.lda + chunk * 8;
    a_lds[i] = r * 128 + ((chunk ^ (r & 7)) << 4);
    w_ptr[i] = W + (n0 + r) * p.K + chunk * 8;
    // LDS row permutation of the 64 weight rows: n_local = q*16 + ni*4 + j  ->  rho = ni*16 + q*4 + j
    const int rho = (((r >> 2) & 3) << 4) + ((r >> 4) << 2) + (r & 3);
    w_lds[i] = 8192 + rho * 128 + ((chunk ^ (rho & 7)) << 4);
  }

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  u32x4 ra[2], rw[2];
  const int KT = (int)(p.K / SM_BK);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    ra[i] = *(const u32x4*)(a_ptr[i]);
    rw[i] = *(const u32x4*)(w_ptr[i]);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    *(u32x4*)(smem + a_lds[i]) = ra[i];
    *(u32x4*)(smem + w_lds[i]) = rw[i];
  }
  __syncthreads();

  // fragment read addresses (within a stage): the wave's 16 rows of A, all 64 rows of W
  const int fr = lane & 15, fq = lane >> 4;
  const int a_rd = (wave * 16 + fr) * 128;
  int w_rd[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w_rd[i] = 8192 + (i * 16 + fr) * 128;
  const int sw = fr & 7;  // (row & 7) == (fr & 7) for every tile row used above

  for (int kt = 0; kt < KT; ++kt) {
    const int cur = (kt & 1) * SM_STAGE;
    const bool more = kt + 1 < KT;
    if (more) {
      const int koff = (kt + 1) * SM_BK;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        ra[i] = *(const u32x4*)(a_ptr[i] + koff);
        rw[i] = *(const u32x4*)(w_ptr[i] + koff);
      }
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int coff = ((s * 4 + fq) ^ sw) << 4;
      const vec8 fa = *(const vec8*)(smem + cur + a_rd + coff);
      vec8 fw[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fw[i] = *(const vec8*)(smem + cur + w_rd[i] + coff);
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) acc[ni] = Ops::mfma16(fw[ni], fa, acc[ni]);
    }
    if (more) {
      const int nxt = ((kt + 1) & 1) * SM_STAGE;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        *(u32x4*)(smem + nxt + a_lds[i]) = ra[i];
        *(u32x4*)(smem + nxt + w_lds[i]) = rw[i];
      }
    }
    __syncthreads();
  }

  // ---- epilogue: lane (fq, fr) holds n = n0 + fq*16 + [0,16) of row m = m0 + wave*16 + fr ----
  const int64_t nb = n0 + fq * 16;
  const int64_t m = m0 + wave * 16 + fr;
  if (m >= p.M) return;
  float v[16];
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[ni * 4 + j] = acc[ni][j] + (p.bias ? p.bias[nb + ni * 4 + j] : 0.0f);
  gemm_store_row<T, EPI>(p, m, nb, v);
}

template <typename T, int EPI>
static void launch_small_one(const GemmParams& p, hipStream_t stream) {
  const unsigned nwg = (unsigned)((p.N / SM_BN) * ((p.M + SM_BM - 1) / SM_BM));
  hipLaunchKernelGGL((gemm_small_kernel<T, EPI>), dim3(nwg), dim3(SM_THREADS), 0, stream, p);
  HIP_CHECK(hipGetLastError());
}

template <typename T>
void launch_gemm_small(const GemmParams& p, int epilogue, hipStream_t stream) {
  if (p.M <= 0) return;
  if (p.N % SM_BN != 0 || p.K % SM_BK != 0 || p.lda % 8 != 0 || p.a_batch_stride % 8 != 0 || p.rows_per_batch <= 0 || p.M >= ((int64_t)1 << 31) ||
      p.N >= ((int64_t)1 << 31) || (p.N / SM_BN) * ((p.M + SM_BM - 1) / SM_BM) >= ((int64_t)1 << 31))
    throw Error(OHW_E_INVALID_ARG, "gemm_small: N and K must be multiples of 64, row strides of 8 elements");
  switch (epilogue) {
    case EPI_BIAS_T: launch_small_one<T, EPI_BIAS_T>(p, stream); break;
    case EPI_BIAS_GELU_T: launch_small_one<T, EPI_BIAS_GELU_T>(p, stream); break;
    case EPI_BIAS_RESID_F32: launch_small_one<T, EPI_BIAS_RESID_F32>(p, stream); break;
    case EPI_GELU_POS_F32: launch_small_one<T, EPI_GELU_POS_F32>(p, stream); break;
    case EPI_F32: launch_small_one<T, EPI_F32>(p, stream); break;
    case EPI_CROSSKV_T: launch_small_one<T, EPI_CROSSKV_T>(p, stream); break;
    default: throw Error(OHW_E_INVALID_ARG, "gemm_small: unknown epilogue");
  }
}

template void launch_gemm_small<bf16_t>(const GemmParams&, int, hipStream_t);
template void launch_gemm_small<f16_t>(const GemmParams&, int, hipStream_t);

}  // namespace ohw
