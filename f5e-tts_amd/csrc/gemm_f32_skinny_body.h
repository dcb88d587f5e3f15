// The body of f5e_gemm_f32_skinny (gemm_f32_skinny.hip has the description), shared with f5e_gemm_f32_w16_skinny
// (gemm_f32_w16.hip): the K-split rule, the chunk ranges, the element-to-MFMA assignment and both summation orders are one
// piece of code, so a 16-bit W widened by its loader (w_load.h) gives the bits of the fp32 launch on the widened copy.
#pragma once
#include "f5e_common.h"
#include "w_load.h"

namespace {

constexpr int SK_ROWS = 16;      // rows of W per workgroup
constexpr int SK_WAVES = 4;      // K ranges per workgroup
constexpr int SK_MAX_KS = 16;

struct SkinnyArgs {
  const float* A;
  const void* W;   // elements of the kernel's loader; ldw in elements
  const float *bias, *addend;
  float *out, *ws;
  int lda, ldw, ld_add, ldo, M, N, K, act, KS;
};

// K-slices per tile: enough workgroups for two per CU, at least four chunks per wave, at most SK_MAX_KS
inline int skinny_ks(int N, int K) {
  const int tiles = (N + SK_ROWS - 1) / SK_ROWS, chunks = (K + 15) / 16;
  int ks = (2 * f5e_cu_count() + tiles - 1) / tiles;
  ks = min(ks, chunks / (4 * SK_WAVES));
  return max(1, min(ks, SK_MAX_KS));
}

__device__ __forceinline__ float skinny_epilogue(const SkinnyArgs& a, float v, int m, int n) {
  if (a.bias) v += a.bias[n];
  if (a.act == F5E_ACT_GELU_ERF) v = gelu_erf_f(v);
  if (a.addend) v += a.addend[(size_t)m * a.ld_add + n];
  return v;
}

// U whole chunks c .. c + U - 1 of a wave's range in one trip (the shorter trips behind the 16-bit kernel's main loop)
template <class WL, int U>
__device__ __forceinline__ void skinny_trip(const typename WL::elem* wp, const float* ap, int c, f32x4& acc) {
  f32x4 wv[U], av[U];
#pragma unroll
  for (int u = 0; u < U; ++u) wv[u] = WL::load4_stream(wp + 16 * (c + u));
#pragma unroll
  for (int u = 0; u < U; ++u) av[u] = *(const f32x4*)(ap + 16 * (c + u));
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][i], wv[u][i], acc, 0, 0, 0);
}

// UNROLL whole chunks per trip: a lane keeps UNROLL loads of W (16 bytes each in fp32, 8 in a 16-bit type) and UNROLL float4
// of A in flight.  The chunks are consumed in ascending order whatever UNROLL is, so it does not touch the bits.
template <class WL, int UNROLL>
__global__ __launch_bounds__(256) void gemm_skinny_kernel(SkinnyArgs a) {
  __shared__ float red[SK_WAVES][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * SK_ROWS, slice = blockIdx.y;
  const int chunks = (a.K + 15) / 16, parts = a.KS * SK_WAVES, part = slice * SK_WAVES + wave;
  const int c_lo = (int)((long long)chunks * part / parts), c_hi = (int)((long long)chunks * (part + 1) / parts);
  const typename WL::elem* wp = (const typename WL::elem*)a.W + (size_t)min(n0 + c16, a.N - 1) * a.ldw + 4 * g;
  const float* ap = a.A + (size_t)min(c16, a.M - 1) * a.lda + 4 * g;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int c = c_lo;
  for (; c + UNROLL <= c_hi && 16 * (c + UNROLL) <= a.K; c += UNROLL) {   // whole chunks: 2 UNROLL loads in flight per lane
    f32x4 wv[UNROLL], av[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) wv[u] = WL::load4_stream(wp + 16 * (c + u));
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) av[u] = *(const f32x4*)(ap + 16 * (c + u));
    // past four chunks hipcc sinks half of the loads between the MFMAs to save registers, which halves the bytes in flight
    // again: all loads of a trip are issued before its first MFMA.  (The fp32 instantiation keeps the schedule it was measured
    // with.)
    if constexpr (UNROLL > 4) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][i], wv[u][i], acc, 0, 0, 0);
  }
  if constexpr (UNROLL > 4) {   // what is left of a range goes in trips of 4 and 2 before the single chunks: a trip is a round trip
    for (; c + 4 <= c_hi && 16 * (c + 4) <= a.K; c += 4) skinny_trip<WL, 4>(wp, ap, c, acc);
    for (; c + 2 <= c_hi && 16 * (c + 2) <= a.K; c += 2) skinny_trip<WL, 2>(wp, ap, c, acc);
  }
  for (; c < c_hi; ++c) {                                         // the rest, and the chunk that K cuts (K % 4 == 0)
    f32x4 wv = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
    if (16 * c + 4 * g + 4 <= a.K) {
      wv = WL::load4_stream(wp + 16 * c);
      av = *(const f32x4*)(ap + 16 * c);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], wv[i], acc, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave][lane][i] = acc[i];
  __syncthreads();
  // thread t owns out[m = t / 16][n0 + t % 16], which lane (g = m / 4, c16 = t % 16) holds in element m % 4
  const int m = tid >> 4, n = n0 + (tid & 15), src = (m >> 2) * 16 + (tid & 15), el = m & 3;
  float v = red[0][src][el];
#pragma unroll
  for (int w = 1; w < SK_WAVES; ++w) v += red[w][src][el];
  if (m >= a.M || n >= a.N) return;
  if (a.KS > 1) a.ws[((size_t)slice * SK_ROWS + m) * a.N + n] = v;
  else a.out[(size_t)m * a.ldo + n] = skinny_epilogue(a, v, m, n);
}

__global__ __launch_bounds__(256) void gemm_skinny_sum_kernel(SkinnyArgs a) {
  const int n = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
  if (n >= a.N) return;
  float v = a.ws[(size_t)m * a.N + n];
  for (int s = 1; s < a.KS; ++s) v += a.ws[((size_t)s * SK_ROWS + m) * a.N + n];
  a.out[(size_t)m * a.ldo + n] = skinny_epilogue(a, v, m, n);
}

inline int skinny_workspace(const char* name, int N, int K, unsigned long long* bytes_out_host) {
  F5E_REQUIRE(bytes_out_host && N > 0 && K > 0, "%s: need N, K > 0 and a place for the answer", name);
  const int ks = skinny_ks(N, K);
  *bytes_out_host = ks > 1 ? (unsigned long long)ks * SK_ROWS * N * sizeof(float) : 0ull;
  return F5E_OK;
}

// Every refusal but the alignment of W (w_align bytes: four elements), then the launch(es).
template <class WL, int UNROLL>
int skinny_launch(const char* name, hipStream_t st, const float* A, int lda, const void* W, int ldw, int w_align, const float* bias,
                  int act, const float* addend, int ld_add, float* out, int ldo, void* workspace,
                  unsigned long long workspace_bytes, int M, int N, int K) {
  F5E_REQUIRE(A && W && out, "%s: null operand", name);
  F5E_REQUIRE(M >= 1 && M <= 16, "%s: built for 1 <= M <= 16 rows (got M=%d); f5e_gemm_f32 takes the rest", name, M);
  F5E_REQUIRE(N >= 1 && K >= 4 && K % 4 == 0 && (long long)N * K < (1ll << 40), "%s: need N >= 1 and K a positive "
              "multiple of 4 (N=%d K=%d)", name, N, K);
  F5E_REQUIRE(act == F5E_ACT_NONE || act == F5E_ACT_GELU_ERF, "%s: act %d is not built (none and GELU_ERF are)", name, act);
  F5E_REQUIRE(lda >= K && ldw >= K && ldo >= N && (!addend || ld_add >= N) && lda % 4 == 0 && ldw % 4 == 0,
              "%s: a leading dimension is smaller than its row, or lda / ldw is not a multiple of 4", name);
  F5E_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)W & (uintptr_t)(w_align - 1)) == 0,
              "%s: A must be 16-byte and W %d-byte aligned", name, w_align);
  const int ks = skinny_ks(N, K);
  F5E_REQUIRE(ks == 1 || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                          workspace_bytes >= (unsigned long long)ks * SK_ROWS * N * sizeof(float)),
              "%s: N=%d K=%d splits K %d ways and needs a 16-byte aligned workspace of f5e_%s_workspace bytes", name, N, K, ks, name);
  const SkinnyArgs a{A, W, bias, addend, out, (float*)workspace, lda, ldw, ld_add, ldo, M, N, K, act, ks};
  const int tiles = (N + SK_ROWS - 1) / SK_ROWS;
  F5E_REQUIRE(tiles <= 0x7fffffff / 2, "%s: N=%d is too large", name, N);
  hipLaunchKernelGGL((gemm_skinny_kernel<WL, UNROLL>), dim3((unsigned)tiles, (unsigned)ks), dim3(256), 0, st, a);
  if (ks > 1) hipLaunchKernelGGL(gemm_skinny_sum_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)M), dim3(256), 0, st, a);
  F5E_LAUNCH_CHECK(name);
  return F5E_OK;
}

}  // namespace
