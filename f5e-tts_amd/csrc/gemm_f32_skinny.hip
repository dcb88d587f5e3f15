// f5e_gemm_f32_skinny: out[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) + addend[m][n] for 1 <= M <= 16 rows, fp32.
//
// A handful of rows against a weight matrix is a read of W and nothing else, so the launch exists to stream W ONCE at a rate
// that involves the whole chip.  f5e_gemm_f32's 32 x 64 tiles give 20 workgroups at N = 1280: here W is cut into tiles of 16
// rows, and where that leaves fewer than two workgroups per CU also along K.
//
//   * a wave owns 16 rows of W and a range of 16-float chunks of K.  Lane (c16, g) loads the float4 W[n0 + c16][16 c + 4 g ..]
//     (a row of the tile is read 64 contiguous bytes at a time, four chunks in flight per lane) and the float4 A[c16][same k];
//     four v_mfma_f32_16x16x4_f32 per chunk leave out[4 g + i][n0 + c16] in the lane.  Rows of A at or beyond M repeat row
//     M - 1 and are never stored, so a row's result does not depend on M.
//   * the four waves of a workgroup take consecutive K ranges of one tile and are summed through LDS in wave order;
//   * with KS > 1 K-slices per tile (N small), slice s writes its partial tile to workspace[s][m][n] and a second launch sums
//     the slices in order s = 0 .. KS - 1 and applies bias, activation and addend.  KS is a function of N, K and the CU count
//     alone.  No floating-point atomics: a launch is bit-reproducible.
//   * addend may alias out: each element is read once and written by the same lane.
#include "f5e_common.h"

namespace {

constexpr int SK_ROWS = 16;      // rows of W per workgroup
constexpr int SK_WAVES = 4;      // K ranges per workgroup
constexpr int SK_MAX_KS = 16;

struct SkinnyArgs {
  const float *A, *W, *bias, *addend;
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

__global__ __launch_bounds__(256) void gemm_skinny_kernel(SkinnyArgs a) {
  __shared__ float red[SK_WAVES][64][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * SK_ROWS, slice = blockIdx.y;
  const int chunks = (a.K + 15) / 16, parts = a.KS * SK_WAVES, part = slice * SK_WAVES + wave;
  const int c_lo = (int)((long long)chunks * part / parts), c_hi = (int)((long long)chunks * (part + 1) / parts);
  const float* wp = a.W + (size_t)min(n0 + c16, a.N - 1) * a.ldw + 4 * g;
  const float* ap = a.A + (size_t)min(c16, a.M - 1) * a.lda + 4 * g;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int c = c_lo;
  for (; c + 4 <= c_hi && 16 * (c + 4) <= a.K; c += 4) {          // four whole chunks: eight loads in flight per lane
    f32x4 wv[4], av[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wv[u] = __builtin_nontemporal_load((const f32x4*)(wp + 16 * (c + u)));
#pragma unroll
    for (int u = 0; u < 4; ++u) av[u] = *(const f32x4*)(ap + 16 * (c + u));
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][i], wv[u][i], acc, 0, 0, 0);
  }
  for (; c < c_hi; ++c) {                                         // the rest, and the chunk that K cuts (K % 4 == 0)
    f32x4 wv = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f};
    if (16 * c + 4 * g + 4 <= a.K) {
      wv = __builtin_nontemporal_load((const f32x4*)(wp + 16 * c));
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

}  // namespace

int f5e_gemm_f32_skinny_workspace(int N, int K, unsigned long long* bytes_out_host) {
  F5E_REQUIRE(bytes_out_host && N > 0 && K > 0, "gemm_f32_skinny_workspace: need N, K > 0 and a place for the answer");
  const int ks = skinny_ks(N, K);
  *bytes_out_host = ks > 1 ? (unsigned long long)ks * SK_ROWS * N * sizeof(float) : 0ull;
  return F5E_OK;
}

int f5e_gemm_f32_skinny(hipStream_t st, const float* A, int lda, const float* W, int ldw, const float* bias, int act,
                        const float* addend, int ld_add, float* out, int ldo, void* workspace, unsigned long long workspace_bytes,
                        int M, int N, int K) {
  F5E_REQUIRE(A && W && out, "gemm_f32_skinny: null operand");
  F5E_REQUIRE(M >= 1 && M <= 16, "gemm_f32_skinny: built for 1 <= M <= 16 rows (got M=%d); f5e_gemm_f32 takes the rest", M);
  F5E_REQUIRE(N >= 1 && K >= 4 && K % 4 == 0 && (long long)N * K < (1ll << 40), "gemm_f32_skinny: need N >= 1 and K a positive "
              "multiple of 4 (N=%d K=%d)", N, K);
  F5E_REQUIRE(act == F5E_ACT_NONE || act == F5E_ACT_GELU_ERF, "gemm_f32_skinny: act %d is not built (none and GELU_ERF are)", act);
  F5E_REQUIRE(lda >= K && ldw >= K && ldo >= N && (!addend || ld_add >= N) && lda % 4 == 0 && ldw % 4 == 0,
              "gemm_f32_skinny: a leading dimension is smaller than its row, or lda / ldw is not a multiple of 4");
  F5E_REQUIRE((((uintptr_t)A | (uintptr_t)W) & 15) == 0, "gemm_f32_skinny: A and W must be 16-byte aligned");
  const int ks = skinny_ks(N, K);
  F5E_REQUIRE(ks == 1 || (workspace && ((uintptr_t)workspace & 15) == 0 &&
                          workspace_bytes >= (unsigned long long)ks * SK_ROWS * N * sizeof(float)),
              "gemm_f32_skinny: N=%d K=%d splits K %d ways and needs a 16-byte aligned workspace of "
              "f5e_gemm_f32_skinny_workspace bytes", N, K, ks);
  const SkinnyArgs a{A, W, bias, addend, out, (float*)workspace, lda, ldw, ld_add, ldo, M, N, K, act, ks};
  const int tiles = (N + SK_ROWS - 1) / SK_ROWS;
  F5E_REQUIRE(tiles <= 0x7fffffff / 2, "gemm_f32_skinny: N=%d is too large", N);
  hipLaunchKernelGGL(gemm_skinny_kernel, dim3((unsigned)tiles, (unsigned)ks), dim3(256), 0, st, a);
  if (ks > 1) hipLaunchKernelGGL(gemm_skinny_sum_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)M), dim3(256), 0, st, a);
  F5E_LAUNCH_CHECK("gemm_f32_skinny");
  return F5E_OK;
}
