// Strided 2-D convolution of the wenet subsampling stacks (Conv2dSubsampling4 / 6 / 8: Conv2d(C, C, 3, 2) and
// Conv2d(C, C, 5, 3) behind the first Conv2d(1, C, 3, 2)) as an IMPLICIT GEMM on the exact-fp32 MFMA
// (v_mfma_f32_16x16x4_f32), channels-last in and out:
//
//   y[b][to][fo][n] = act( bias[n] + sum_{i < kt, j < kf, c < C} x[b][to s + i][fo s + j][c] * w[n][i][j][c] )
//
//   M = B T_out F_out rows, N = C output channels, K = kt kf C.
//
// No im2col matrix exists: row m = (b, to, fo) of the A operand is gathered by the loader.  Channels-last makes the kf taps
// of one kernel row ONE contiguous run of kf C floats (x[b][to s + i][fo s .. fo s + kf - 1][:]), so a row of A is kt runs,
// the run i starting i * F_in * C floats behind the row's base; K-offset k lies in run k / (kf C).  C % 4 == 0 keeps every
// 16-byte chunk inside one run.  The weight is repacked on the host to [N][kt][kf][C] = a plain [N][K] matrix.
//
// The pipeline is gemm_f32.hip's LDS-DMA ring (global_load_lds_dwordx4 into an NSTAGE-deep ring, counted vmcnt, one raw
// s_barrier per K-step of 64 floats, chunk ^ (row & 15) swizzle on the source address and on the ds_read_b128); only the
// A-side source address differs.  Workspace: none.  T_out / F_out / N tails are predicated: rows m >= M and channels n >= N
// are loaded from a clamped (valid) address and never stored.
#include "f5e_common.h"

namespace {

struct ConvSubArgs {
  const float* x; const float* w; const float* bias; float* y;
  int T_in, F_in, F_out, TF;  // TF = T_out * F_out
  int C, stride, seg, row_stride;  // seg = kf * C floats per kernel row, row_stride = F_in * C floats between kernel rows
  int act;
  int M, N, K;
  int tiles_m;
};

template <int BM, int BN, int WGM, int WGN, int NSTAGE>
__global__ __launch_bounds__(256) void conv2d_sub_kernel(ConvSubArgs a) {
  constexpr int BK = 64, NT = 256, ROWB = BK * 4;
  constexpr int A_BYTES = BM * ROWB, W_BYTES = BN * ROWB, STAGE = A_BYTES + W_BYTES;
  constexpr int WM = BM / WGM, WN = BN / WGN, TM = WM / 16, TN = WN / 16;
  constexpr int A_IT = BM * 16 / NT, W_IT = BN * 16 / NT, LPT = A_IT + W_IT;
  static_assert(WGM * WGN == 4 && TM >= 1 && TN >= 1 && A_IT >= 1 && W_IT >= 1, "tile / wave layout");
  static_assert((NSTAGE - 2) * LPT <= 63, "vmcnt is a 6-bit counter");
  extern __shared__ __attribute__((aligned(16))) char smem_sub[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile_n = blockIdx.x / a.tiles_m, tile_m = blockIdx.x - tile_n * a.tiles_m;
  const int m0 = tile_m * BM, n0 = tile_n * BN;

  const float* a_row[A_IT];  // x[b][to s][fo s][0] of the thread's row
  const float* w_row[W_IT];
  int a_k[A_IT], w_k[W_IT];  // first k of the thread's chunk inside a K-tile
#pragma unroll
  for (int j = 0; j < A_IT; ++j) {
    const int i = tid + NT * j, row = i >> 4, c = (i & 15) ^ (row & 15);
    const int m = min(m0 + row, a.M - 1);
    const int b = m / a.TF, r = m - b * a.TF, to = r / a.F_out, fo = r - to * a.F_out;
    a_row[j] = a.x + ((size_t)(b * a.T_in + to * a.stride) * a.F_in + fo * a.stride) * a.C;
    a_k[j] = c * 4;
  }
#pragma unroll
  for (int j = 0; j < W_IT; ++j) {
    const int i = tid + NT * j, row = i >> 4, c = (i & 15) ^ (row & 15);
    w_row[j] = a.w + (size_t)min(n0 + row, a.N - 1) * a.K;
    w_k[j] = c * 4;
  }
  auto dma = [](const void* g, void* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
  };
  // chunks of the last K-tile that start at k >= K are fetched from the row start instead (a valid address) and overwritten
  // with zeros by their owner once they have landed
  auto stage = [&](int buf, int kt) {
    char* base = smem_sub + buf * STAGE;
#pragma unroll
    for (int j = 0; j < A_IT; ++j) {
      int k = kt * BK + a_k[j];
      if (k >= a.K) k = 0;
      const int run = k / a.seg;
      dma(a_row[j] + (size_t)run * a.row_stride + (k - run * a.seg), base + (wave * 64 + NT * j) * 16);
    }
#pragma unroll
    for (int j = 0; j < W_IT; ++j) {
      const int k = kt * BK + w_k[j];
      dma(w_row[j] + (k < a.K ? k : 0), base + A_BYTES + (wave * 64 + NT * j) * 16);
    }
  };

  const int wm0 = (wave / WGN) * WM, wn0 = (wave % WGN) * WN;
  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int KT = (a.K + BK - 1) / BK;
#pragma unroll
  for (int s = 0; s < NSTAGE - 1; ++s)
    if (s < KT) stage(s, s);
  int buf = 0, nbuf = NSTAGE - 1;
  for (int kt = 0; kt < KT; ++kt) {
    const int rem = KT - 1 - kt;
    switch (rem < NSTAGE - 2 ? rem : NSTAGE - 2) {  // tile kt landed; that many younger stages may stay in flight
      case 0: asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(0) : "memory"); break;
      case 1: asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(LPT) : "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(2 * LPT) : "memory"); break;
    }
    if (rem == 0 && (a.K & (BK - 1))) {  // ragged tail: own chunks past K become zeros (own DMAs have landed: vmcnt(0))
      char* base = smem_sub + buf * STAGE;
#pragma unroll
      for (int j = 0; j < A_IT; ++j)
        if (kt * BK + a_k[j] >= a.K) *(f32x4*)(base + (tid + NT * j) * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < W_IT; ++j)
        if (kt * BK + w_k[j] >= a.K) *(f32x4*)(base + A_BYTES + (tid + NT * j) * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const char* As = smem_sub + buf * STAGE;
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
    // fragment reads before the next tile's LDS-DMAs, as in gemm_f32.hip
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

  // a lane owns 4 consecutive channels of one output position; N % 4 == 0, y and bias 16-byte aligned (host check)
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    const int m = m0 + wm0 + j * 16 + fr;
    if (m >= a.M) continue;
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int n = n0 + wn0 + i * 16 + fq * 4;
      if (n >= a.N) continue;
      f32x4 v = acc[i][j];
      if (a.bias) v += *(const f32x4*)(a.bias + n);
      if (a.act != F5E_ACT_NONE) { v[0] = apply_act(v[0], a.act); v[1] = apply_act(v[1], a.act); v[2] = apply_act(v[2], a.act); v[3] = apply_act(v[3], a.act); }
      *(f32x4*)(a.y + (size_t)m * a.N + n) = v;
    }
  }
}

template <int BM, int BN, int WGM, int WGN, int NSTAGE>
int launch_sub(ConvSubArgs& a, hipStream_t st) {
  a.tiles_m = (a.M + BM - 1) / BM;
  const int grid = a.tiles_m * ((a.N + BN - 1) / BN);
  constexpr int lds_max = NSTAGE * (BM + BN) * 256;
  static F5eDeviceOnce lds_once;  // > 64 KiB of dynamic LDS needs the opt-in attribute, per device
  if (lds_max > 65536) F5E_OPT_IN_LDS(lds_once, (conv2d_sub_kernel<BM, BN, WGM, WGN, NSTAGE>), lds_max);
  hipLaunchKernelGGL((conv2d_sub_kernel<BM, BN, WGM, WGN, NSTAGE>), dim3(grid), dim3(256), lds_max, st, a);
  F5E_LAUNCH_CHECK("conv2d_sub_f32");
  return F5E_OK;
}

}  // namespace

extern "C" int f5e_conv2d_sub_f32(hipStream_t st, const float* x, const float* w, const float* bias, float* y, int B,
                                  int T_in, int F_in, int C, int kt, int kf, int stride, int act) {
  F5E_REQUIRE(x && w && y, "conv2d_sub_f32: null operand");
  F5E_REQUIRE(B > 0 && C > 0 && C % 16 == 0, "conv2d_sub_f32: B > 0 and C a positive multiple of 16 (B=%d C=%d)", B, C);
  F5E_REQUIRE(kt >= 1 && kf >= 1 && kt <= 8 && kf <= 8 && stride >= 1, "conv2d_sub_f32: kernel 1..8, stride >= 1 (kt=%d kf=%d s=%d)",
              kt, kf, stride);
  F5E_REQUIRE(T_in >= kt && F_in >= kf, "conv2d_sub_f32: input [%d, %d] is smaller than the kernel [%d, %d]", T_in, F_in, kt, kf);
  F5E_REQUIRE(act == F5E_ACT_NONE || act == F5E_ACT_RELU, "conv2d_sub_f32: act must be none or relu");
  F5E_REQUIRE((((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) & 15) == 0, "conv2d_sub_f32: operands must be 16-byte aligned");
  const int T_out = (T_in - kt) / stride + 1, F_out = (F_in - kf) / stride + 1;
  const long long in_pos = (long long)B * T_in * F_in, rows = (long long)B * T_out * F_out;
  F5E_REQUIRE(in_pos < (1ll << 31) && rows < (1ll << 31) - 64, "conv2d_sub_f32: B * T * F exceeds the 31-bit position index");
  ConvSubArgs a{};
  a.x = x; a.w = w; a.bias = bias; a.y = y; a.T_in = T_in; a.F_in = F_in; a.F_out = F_out; a.TF = T_out * F_out;
  a.C = C; a.stride = stride; a.seg = kf * C; a.row_stride = F_in * C; a.act = act;
  a.M = (int)rows; a.N = C; a.K = kt * kf * C;
  if (((a.M + 63) / 64) * ((a.N + 63) / 64) < 128) return launch_sub<32, 64, 2, 2, 4>(a, st);
  return launch_sub<64, 64, 2, 2, 3>(a, st);
}
