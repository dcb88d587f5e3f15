// Exact-fp32 MFMA GEMM (v_mfma_f32_16x16x4_f32) for everything that runs once per sample() call or on the ODE
// state itself, where the reference computes in fp32 and bf16 rounding would cost parity for no speed:
//   time MLP + all AdaLN tables (modules.py:721-731, :311, :332), TextEmbedding / ConvNeXtV2 pointwise convs
//   (backbones/dit.py:54-87, modules.py:265-268), PPGEmbedding linears/convs (dit.py:121-138), the x-part of the
//   input projection (dit.py:173-175) and the Vocos backbone / head linears.
//
//   C[m][n] = epi( sum_k actA(A[m % a_rows][k]) * W[n][k] )
//   epi(v)  = ((act(v + bias[n])) * ch_scale[n] + addend[m % add_rows][n]) * row_scale[m]
//
// The plain kernel (64x64 tile, register-staged) lives in gemm_f32_tile.h, which gemm_f32_w16.hip shares.
#include "f5e_common.h"
#include "gemm_f32_tile.h"

namespace {

// ---- LDS-DMA variant for every call without an A-side activation (input projection, TextEmbedding / Vocos convs, head) ----
// Same ring as gemm_bf16.hip: global_load_lds_dwordx4 into an NSTAGE-deep LDS ring, counted vmcnt + one raw
// s_barrier per K-step of 64 floats (256-byte rows, 16 chunks of 16 B; chunk ^ (row & 15) on the source address and
// on the ds_read_b128 -> each 16-lane group covers all 64 banks once).  A lane (fr, fq) reads 4 consecutive k of its
// row and feeds them to 4 MFMAs; both operands use the same k permutation, so every k is visited exactly once.
// The plain kernel takes ~1.4 us per 16-wide K step (exposed global latency + 2 barriers): 45 us for
// 281 x 1536 x 512; this one ~8 us.
// The fields the prologue needs before its first LDS-DMA come once more as LEADING SCALAR parameters (11 dwords, preloaded
// into SGPRs at wave launch: f5e_common.h, f5e_kernarg_late); the struct's kernarg lines are requested behind the prologue's
// DMAs, under the first tile's flight.  One list for the signature and the launcher:
#define F5E_GEMM32_HOT_PARAMS                                                                                            \
  const float *h_A, const float *h_W, int h_lda, int h_ldw, int h_a_rows, int h_M, int h_N, int h_K, int h_tiles_m
#define F5E_GEMM32_HOT_ARGS(a) (a).A, (a).W, (a).lda, (a).ldw, (a).a_rows, (a).M, (a).N, (a).K, (a).tiles_m
enum { F5E_GEMM32_HOT_DWORDS = 11 };
template <int BM, int BN, int WGM, int WGN, int NSTAGE>
__global__ __launch_bounds__(256) void gemm_f32_dma_kernel(F5E_GEMM32_HOT_PARAMS, Gemm32Args a) {
  constexpr int BK = 64, NT = 256, ROWB = BK * 4;
  constexpr int A_BYTES = BM * ROWB, W_BYTES = BN * ROWB, STAGE = A_BYTES + W_BYTES;
  constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 16, TN = WN / 16;
  constexpr int A_IT = BM * 16 / NT, W_IT = BN * 16 / NT, LPT = A_IT + W_IT;
  static_assert(WGM * WGN == 4 && TM >= 1 && TN >= 1 && A_IT >= 1 && W_IT >= 1, "tile / wave layout");
  static_assert((NSTAGE - 2) * LPT <= 63, "vmcnt is a 6-bit counter");
  extern __shared__ __attribute__((aligned(16))) char smem32[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile_n = blockIdx.x / h_tiles_m, tile_m = blockIdx.x - tile_n * h_tiles_m;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const float* a_src[A_IT];
  const float* w_src[W_IT];
  int a_k[A_IT], w_k[W_IT];  // first k of the thread's chunk inside a K-tile (for the ragged last tile)
#pragma unroll
  for (int j = 0; j < A_IT; ++j) {
    const int i = tid + NT * j, row = i >> 4, c = (i & 15) ^ (row & 15);
    a_src[j] = h_A + (size_t)(min(m0 + row, h_M - 1) % h_a_rows) * h_lda + c * 4;
    a_k[j] = c * 4;
  }
#pragma unroll
  for (int j = 0; j < W_IT; ++j) {
    const int i = tid + NT * j, row = i >> 4, c = (i & 15) ^ (row & 15);
    w_src[j] = h_W + (size_t)min(n0 + row, h_N - 1) * h_ldw + c * 4;
    w_k[j] = c * 4;
  }
  auto dma = [](const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
  };
  // K % 64 != 0 (K % 4 == 0 always): chunks of the last K-tile that start at k >= K are fetched from the row start
  // instead (any valid address: no out-of-bounds read) and overwritten with zeros by their owner once they have landed
  auto stage = [&](int buf, int kt) {
    char* base = smem32 + buf * STAGE;
#pragma unroll
    for (int j = 0; j < A_IT; ++j)
      dma(kt * BK + a_k[j] < h_K ? a_src[j] + kt * BK : a_src[j] - a_k[j], base + (wave * 64 + NT * j) * 16);
#pragma unroll
    for (int j = 0; j < W_IT; ++j)
      dma(kt * BK + w_k[j] < h_K ? w_src[j] + kt * BK : w_src[j] - w_k[j], base + A_BYTES + (wave * 64 + NT * j) * 16);
  };

  const int wm0 = (wave / WGN) * WM, wn0 = (wave % WGN) * WN;
  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int KT = (h_K + BK - 1) / BK;
#pragma unroll
  for (int s = 0; s < NSTAGE - 1; ++s)
    if (s < KT) stage(s, s);
  // every wave waits below for its first tile anyway: the struct's (cold) kernarg lines are requested here, all at once
  asm volatile("" ::"s"(a.vec), "s"(a.addend), "s"(a.ld_add), "s"(a.add_rows), "s"(a.row_scale), "s"(a.bias), "s"(a.act),
               "s"(a.ch_scale), "s"(a.out), "s"(a.ldo), "s"(a.out_bf16), "s"(a.ldo_bf16));
  int buf = 0, nbuf = NSTAGE - 1;
  for (int kt = 0; kt < KT; ++kt) {
    const int rem = KT - 1 - kt;
    switch (rem < NSTAGE - 2 ? rem : NSTAGE - 2) {  // tile kt landed; that many younger stages may stay in flight
      case 0: asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(0) : "memory"); break;
      case 1: asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPT) : "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * LPT) : "memory"); break;
    }
    if (rem == 0 && (a.K & (BK - 1))) {  // ragged tail: own chunks past K become zeros (own DMAs have landed: vmcnt(0))
      char* base = smem32 + buf * STAGE;
#pragma unroll
      for (int j = 0; j < A_IT; ++j)
        if (kt * BK + a_k[j] >= a.K) *(f32x4*)(base + (tid + NT * j) * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < W_IT; ++j)
        if (kt * BK + w_k[j] >= a.K) *(f32x4*)(base + A_BYTES + (tid + NT * j) * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const char* As = smem32 + buf * STAGE;
    const char* Ws = As + A_BYTES;
    f32x4 xf[TM], wf[TN];
    auto reads = [&](int g) {
      const int c = g * 4 + fq;
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int row = wm0 + j * 16 + fr;
        xf[j] = *(const f32x4*)(As + row * ROWB + ((c ^ (row & 15)) << 4));
      }
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int row = wn0 + i * 16 + fr;
        wf[i] = *(const f32x4*)(Ws + row * ROWB + ((c ^ (row & 15)) << 4));
      }
    };
    // the first fragment reads go out BEFORE the next tile's LDS-DMAs: a DMA costs the wave 100+ cycles of issue while the
    // CU's address path is busy, and reads issued behind it (the order of rounds 1-2) wait that long (gemm_bf16.hip)
    reads(0);
    if (kt + NSTAGE - 1 < KT) stage(nbuf, kt + NSTAGE - 1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (g > 0) reads(g);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
          for (int j = 0; j < TM; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i][r], xf[j][r], acc[i][j], 0, 0, 0);
    }
    buf = (buf + 1 == NSTAGE) ? 0 : buf + 1;
    nbuf = (nbuf + 1 == NSTAGE) ? 0 : nbuf + 1;
  }

  if (a.vec) {
    // N, leading dimensions and pointers are 16-byte friendly (host check): quads of 4 columns move as one piece and
    // the addend rows are requested together, ahead of the arithmetic (one round trip instead of sixteen)
    f32x4 add[TN][TM];
    if (a.addend) {
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        const int m = min(m0 + wm0 + j * 16 + fr, a.M - 1);
        const float* ap = a.addend + (size_t)(m % a.add_rows) * a.ld_add;
#pragma unroll
        for (int i = 0; i < TN; ++i) add[i][j] = *(const f32x4*)(ap + min(n0 + wn0 + i * 16 + fq * 4, a.N - 4));
      }
    }
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int m = m0 + wm0 + j * 16 + fr;
      if (m >= a.M) continue;
      const float rs = a.row_scale ? a.row_scale[m] : 1.0f;
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int n = n0 + wn0 + i * 16 + fq * 4;
        if (n >= a.N) continue;
        f32x4 v = acc[i][j];
        if (a.bias) v += *(const f32x4*)(a.bias + n);
        if (a.act != F5E_ACT_NONE) { v[0] = apply_act(v[0], a.act); v[1] = apply_act(v[1], a.act); v[2] = apply_act(v[2], a.act); v[3] = apply_act(v[3], a.act); }
        if (a.ch_scale) v *= *(const f32x4*)(a.ch_scale + n);
        if (a.addend) v += add[i][j];
        v *= rs;
        if (a.out) *(f32x4*)(a.out + (size_t)m * a.ldo + n) = v;
        if (a.out_bf16) *(bf16x4*)(a.out_bf16 + (size_t)m * a.ldo_bf16 + n) = f2bf4(v[0], v[1], v[2], v[3]);
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    const int m = m0 + wm0 + j * 16 + fr;
    if (m >= a.M) continue;
    const float rs = a.row_scale ? a.row_scale[m] : 1.0f;
#pragma unroll
    for (int i = 0; i < TN; ++i) {
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

template <int BM, int BN, int WGM, int WGN, int NSTAGE>
int launch_dma(Gemm32Args& a, hipStream_t st) {
  a.tiles_m = (a.M + BM - 1) / BM;
  const int grid = a.tiles_m * ((a.N + BN - 1) / BN);
  constexpr int lds_max = NSTAGE * (BM + BN) * 256;
  static F5eDeviceOnce lds_once;  // > 64 KiB of dynamic LDS needs the opt-in attribute, per device (host-only call)
  if (lds_max > 65536) F5E_OPT_IN_LDS(lds_once, (gemm_f32_dma_kernel<BM, BN, WGM, WGN, NSTAGE>), lds_max);
  // a K of fewer tiles than ring slots never re-stages: slots >= KT are untouched, so they need not exist.  The per-step
  // input projection (K = 100: 2 tiles) then takes 64 instead of 96 KiB and two workgroups share a CU.
  const int kt = (a.K + 63) / 64;
  const int lds = (kt < NSTAGE ? kt : NSTAGE) * (BM + BN) * 256;
  hipLaunchKernelGGL((gemm_f32_dma_kernel<BM, BN, WGM, WGN, NSTAGE>), dim3(grid), dim3(256), lds, st, F5E_GEMM32_HOT_ARGS(a), a);
  F5E_LAUNCH_CHECK("gemm_f32_dma");
  return F5E_OK;
}

}  // namespace

extern "C" int f5e_gemm_f32(hipStream_t st, const float* A, int lda, int a_rows, int a_act, const float* W, int ldw,
                            const float* bias, int act, const float* ch_scale, const float* addend, int ld_add,
                            int add_rows, const float* row_scale, float* out, int ldo, void* out_bf16, int ldo_bf16,
                            int M, int N, int K) {
  Gemm32Args a;
  const int rc = gemm32_args("gemm_f32", a, A, lda, a_rows, a_act, W, ldw, bias, act, ch_scale, addend, ld_add, add_rows, row_scale,
                             out, ldo, out_bf16, ldo_bf16, M, N, K);
  if (rc != F5E_OK) return rc;
  if (gemm32_dma_order(a_act, A, W)) {
    // few tiles: halve BM so more CUs take part (these GEMMs have M of a few hundred rows)
    if (((M + 63) / 64) * ((N + 63) / 64) < 128) return launch_dma<32, 64, 2, 2, 4>(a, st);
    return launch_dma<64, 64, 2, 2, 3>(a, st);
  }
  return gemm32_launch_tile<WLoadF32, false>("gemm_f32", a, st);
}
