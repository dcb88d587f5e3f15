// The register-staged 64 x 64 tile of the exact-fp32 GEMM (gemm_f32.hip has the formula), shared by f5e_gemm_f32 (fp32 W) and
// f5e_gemm_f32_w16 (16-bit W, widened by the loader: w_load.h).  4 waves (2 x 2), K-step 16, LDS rows padded to 17 floats
// (conflict-free ds_read_b32).  Operands swapped like gemm_bf16.hip: a lane owns 4 consecutive n of one row m.
//
// DMA_ORDER: which k an MFMA's four slots hold.  false: MFMA kk of a K-step takes k = 4 kk + slot, the order f5e_gemm_f32's
// plain kernel always had.  true: MFMA r takes k = 4 slot + r, the order of gemm_f32_dma_kernel (a lane reads 4 consecutive k
// and feeds them to 4 MFMAs), so that a 16-bit W, which cannot ride the LDS-DMA ring, still gives that kernel's bits.  Only
// the place of an element inside its LDS row differs; A and W move together.
#pragma once
#include "f5e_common.h"
#include "w_load.h"

namespace {

struct Gemm32Args {
  const float* A; int lda; int a_rows; int a_act;
  const float* W; int ldw;  // with a 16-bit loader: that type's elements behind the pointer, ldw in elements
  const float* bias;
  int act;
  const float* ch_scale;
  const float* addend; int ld_add; int add_rows;
  const float* row_scale;
  float* out; int ldo;
  bf16* out_bf16; int ldo_bf16;
  int M, N, K;
  int tiles_m;
  int vec;  // epilogue may move 4 columns at a time (alignment checked on the host)
};

template <class WL, bool DMA_ORDER>
__global__ __launch_bounds__(256) void gemm_f32_kernel(Gemm32Args a) {
  constexpr int BK = 16, LDS_ROW = 17;
  __shared__ float As[2][64 * LDS_ROW];
  __shared__ float Ws[2][64 * LDS_ROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile_n = blockIdx.x / a.tiles_m, tile_m = blockIdx.x - tile_n * a.tiles_m;
  const int m0 = tile_m * 64, n0 = tile_n * 64;

  const int lrow = tid >> 2, lc = (tid & 3) * 4;
  const int am = min(m0 + lrow, a.M - 1) % a.a_rows;
  const int wn = min(n0 + lrow, a.N - 1);
  const float* ap = a.A + (size_t)am * a.lda + lc;
  const typename WL::elem* wp = (const typename WL::elem*)(const void*)a.W + (size_t)wn * a.ldw + lc;

  // K % 4 == 0 and lc % 4 == 0: a group of four is either fully inside or fully outside [0, K)
  auto gload = [&](const float* p, int k0) -> f32x4 {
    if (k0 + lc < a.K) return *(const f32x4*)(p + k0);
    return f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto wload = [&](int k0) -> f32x4 {
    if (k0 + lc < a.K) return WL::load4(wp + k0);
    return f32x4{0.f, 0.f, 0.f, 0.f};
  };
  auto sstore = [&](float* dst, f32x4 v) {
    if constexpr (DMA_ORDER) {
      float* d = dst + lrow * LDS_ROW + (tid & 3);
      d[0] = v[0]; d[4] = v[1]; d[8] = v[2]; d[12] = v[3];
    } else {
      float* d = dst + lrow * LDS_ROW + lc;
      d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    }
  };

  const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int KT = (a.K + BK - 1) / BK;
  f32x4 ra = gload(ap, 0), rw = wload(0);
  if (a.a_act) { ra[0] = apply_act(ra[0], a.a_act); ra[1] = apply_act(ra[1], a.a_act);
                 ra[2] = apply_act(ra[2], a.a_act); ra[3] = apply_act(ra[3], a.a_act); }
  sstore(As[0], ra);
  sstore(Ws[0], rw);
  __syncthreads();
  for (int kt = 0; kt < KT; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < KT) {
      ra = gload(ap, (kt + 1) * BK);
      rw = wload((kt + 1) * BK);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      float xf[2], wf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) xf[j] = As[buf][(wm0 + j * 16 + fr) * LDS_ROW + kk * 4 + fq];
#pragma unroll
      for (int i = 0; i < 2; ++i) wf[i] = Ws[buf][(wn0 + i * 16 + fr) * LDS_ROW + kk * 4 + fq];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i], xf[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < KT) {
      if (a.a_act) { ra[0] = apply_act(ra[0], a.a_act); ra[1] = apply_act(ra[1], a.a_act);
                     ra[2] = apply_act(ra[2], a.a_act); ra[3] = apply_act(ra[3], a.a_act); }
      sstore(As[buf ^ 1], ra);
      sstore(Ws[buf ^ 1], rw);
    }
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wm0 + j * 16 + fr;
    if (m >= a.M) continue;
    const float rs = a.row_scale ? a.row_scale[m] : 1.0f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = n0 + wn0 + i * 16 + fq * 4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = n + r;
        if (nn >= a.N) continue;
        float v = acc[i][j][r];
        if (a.bias) v += a.bias[nn];
        v = apply_act(v, a.act);
        if (a.ch_scale) v *= a.ch_scale[nn];
        if (a.addend) v += a.addend[(size_t)(m % a.add_rows) * a.ld_add + nn];
        v *= rs;
        if (a.out) a.out[(size_t)m * a.ldo + nn] = v;
        if (a.out_bf16) a.out_bf16[(size_t)m * a.ldo_bf16 + nn] = (bf16)v;
      }
    }
  }
}

// The refusals of the family's entry points (W's own alignment stays with each) and the argument record they launch with.
inline int gemm32_args(const char* name, Gemm32Args& a, const float* A, int lda, int a_rows, int a_act, const void* W, int ldw,
                       const float* bias, int act, const float* ch_scale, const float* addend, int ld_add, int add_rows,
                       const float* row_scale, float* out, int ldo, void* out_bf16, int ldo_bf16, int M, int N, int K) {
  F5E_REQUIRE(A && W && (out || out_bf16), "%s: null operand", name);
  F5E_REQUIRE(M > 0 && N > 0 && K > 0, "%s: empty problem M=%d N=%d K=%d", name, M, N, K);
  F5E_REQUIRE(K % 4 == 0 && lda % 4 == 0 && ldw % 4 == 0, "%s: K, lda, ldw must be multiples of 4 (K=%d)", name, K);
  F5E_REQUIRE(a_rows > 0, "%s: a_rows must be positive", name);
  if (addend) F5E_REQUIRE(add_rows > 0, "%s: add_rows must be positive", name);
  // rows of an operand that is written, or read once per output element, must not overlap (A and W rows may)
  if (M > 1) {
    if (out) F5E_REQUIRE(ldo >= N, "%s: ldo=%d must be at least N=%d", name, ldo, N);
    if (out_bf16) F5E_REQUIRE(ldo_bf16 >= N, "%s: ldo_bf16=%d must be at least N=%d", name, ldo_bf16, N);
    if (addend && add_rows > 1) F5E_REQUIRE(ld_add >= N, "%s: ld_add=%d must be at least N=%d", name, ld_add, N);
  }
  F5E_REQUIRE(lda >= 0 && ldw >= 0, "%s: lda, ldw must not be negative", name);
  a = Gemm32Args{};
  a.A = A; a.lda = lda; a.a_rows = a_rows; a.a_act = a_act; a.W = (const float*)W; a.ldw = ldw; a.bias = bias; a.act = act;
  a.ch_scale = ch_scale; a.addend = addend; a.ld_add = ld_add; a.add_rows = add_rows > 0 ? add_rows : 1;
  a.row_scale = row_scale; a.out = out; a.ldo = ldo; a.out_bf16 = (bf16*)out_bf16; a.ldo_bf16 = ldo_bf16;
  a.M = M; a.N = N; a.K = K;
  a.vec = N % 4 == 0 && N >= 4 && ldo % 4 == 0 && ldo_bf16 % 4 == 0 && ld_add % 4 == 0 &&
          (((uintptr_t)bias | (uintptr_t)ch_scale | (uintptr_t)addend | (uintptr_t)out) & 15) == 0 && ((uintptr_t)out_bf16 & 7) == 0;
  return F5E_OK;
}

// f5e_gemm_f32 takes its LDS-DMA kernel, whose MFMAs hold k in DMA_ORDER, exactly then (K % 4 == 0 is checked above)
inline bool gemm32_dma_order(int a_act, const float* A, const void* W_f32) {
  return a_act == F5E_ACT_NONE && (((uintptr_t)A | (uintptr_t)W_f32) & 15) == 0;
}

template <class WL, bool DMA_ORDER>
int gemm32_launch_tile(const char* name, Gemm32Args& a, hipStream_t st) {
  a.tiles_m = (a.M + 63) / 64;
  const int grid = a.tiles_m * ((a.N + 63) / 64);
  hipLaunchKernelGGL((gemm_f32_kernel<WL, DMA_ORDER>), dim3(grid), dim3(256), 0, st, a);
  F5E_LAUNCH_CHECK(name);
  return F5E_OK;
}

}  // namespace
