// BigVGAN-v2 generator kernels (vocoder_bigvgan.py): channels-last [B][L][C] activations, fp32 residual stream.
//
// f5e_bigvgan_act: Activation1d (anti-aliased SnakeBeta) as one stencil.  Per channel c and output row t:
//   up[2a]   = 2 sum_k x[a-3+k] fu[11-2k],  up[2a+1] = 2 sum_k x[a-2+k] fu[10-2k]   (k < 6, x index clamped to [0, L):
//              replicate-pad 5, 2 * conv_transpose1d(stride 2, 12 taps), crop [15:-15])
//   s[i]     = up[i] + inv_beta[c] sin^2(alpha[c] up[i])                           (alpha, inv_beta prepared on the host)
//   y[t]     = sum_m fd[m] s[clamp(2t + m - 5, 0, 2L - 1)]                          (replicate-pad (5, 6), stride-2 conv)
//   fp32 in, bf16 (conv operand) or fp32 (conv_post operand) out.  A thread walks R consecutive rows of one channel, so
//   each up-sample / sine is computed once per 2 output rows' worth of new input instead of 12 times.
// f5e_bigvgan_conv: dilated Conv1d as an implicit GEMM on v_mfma_f32_32x32x16_bf16.  M = rows of one sequence (tiles never
//   straddle sequences), N = C_out, K = k * C_in.  Per 32-wide C_in chunk the input tile plus its dilated halo
//   (BM + (k-1) d rows) is staged in LDS once and every tap is a row offset into it; the chunk's weights for all k taps
//   sit beside it.  Epilogue: + bias, + residual (x + t), and / or the AMP stage mean (sum = [sum +] scale * value).
//   The transposed convolutions of the upsamplers run through the same kernel: vocoder_bigvgan.py repacks a
//   ConvTranspose1d(stride u) as a 3-tap conv with N = u * C_out, whose [L][u * C_out] output IS [L * u][C_out].
// f5e_bigvgan_post: conv_post (C -> 1, k taps, fp32) + clamp(-1, 1) or tanh -> waveform fp32 [B][L].
#include "f5e_common.h"

namespace {

// ---------------------------------------------------------------- Activation1d
constexpr int ACT_R = 8;   // output rows per thread

template <typename OUT>
__device__ __forceinline__ void store_act(OUT* p, float v);
template <>
__device__ __forceinline__ void store_act<float>(float* p, float v) { *p = v; }
template <>
__device__ __forceinline__ void store_act<bf16>(bf16* p, float v) { *p = (bf16)v; }

template <typename OUT>
__global__ __launch_bounds__(256) void act_kernel(const float* __restrict__ x, OUT* __restrict__ y,
                                                  const float* __restrict__ alpha, const float* __restrict__ inv_beta,
                                                  const float* __restrict__ f_up, const float* __restrict__ f_dn, int L,
                                                  int C, int chunks, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long long rc = idx / C;
  const int chunk = (int)(rc % chunks);
  const int b = (int)(rc / chunks);
  const int t0 = chunk * ACT_R;
  const float* xb = x + (size_t)b * L * C + c;
  float fu[12], fd[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) { fu[k] = f_up[k]; fd[k] = f_dn[k]; }
  const float al = alpha[c], ib = inv_beta[c];
  // s[q] = snake(up(clamp(2 t0 - 5 + q, 0, 2L - 1))), q < 2R + 10
  float s[2 * ACT_R + 10];
  if (2 * t0 - 5 >= 0 && 2 * t0 + 2 * ACT_R + 4 <= 2 * L - 1) {
    // interior rows: no up-sample index is clamped, so every tap is a static offset into the R + 10 input rows
    // [t0 - 5, t0 + R + 4] (clamped to [0, L) on load), read once instead of 6 times per up-sample
    float xw[ACT_R + 10];
#pragma unroll
    for (int j = 0; j < ACT_R + 10; ++j) {
      const int tj = t0 - 5 + j;
      xw[j] = xb[(size_t)(tj < 0 ? 0 : (tj > L - 1 ? L - 1 : tj)) * C];
    }
#pragma unroll
    for (int q = 0; q < 2 * ACT_R + 10; ++q) {
      const int odd = (q - 5) & 1;
      const int a0 = ((q - 5) >> 1) + 2 + odd;   // first input row of up-sample 2 t0 - 5 + q, relative to t0 - 5
      float u = 0.f;
#pragma unroll
      for (int k = 0; k < 6; ++k) u += xw[a0 + k] * (odd ? fu[10 - 2 * k] : fu[11 - 2 * k]);
      u *= 2.f;
      const float sn = sinf(al * u);
      s[q] = u + ib * (sn * sn);
    }
  } else {
#pragma unroll
    for (int q = 0; q < 2 * ACT_R + 10; ++q) {
      int i = 2 * t0 - 5 + q;
      i = i < 0 ? 0 : (i > 2 * L - 1 ? 2 * L - 1 : i);
      const int odd = i & 1;
      const int a0 = (i >> 1) - 3 + odd;
      float u = 0.f;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        int j = a0 + k;
        j = j < 0 ? 0 : (j > L - 1 ? L - 1 : j);
        u += xb[(size_t)j * C] * (odd ? fu[10 - 2 * k] : fu[11 - 2 * k]);
      }
      u *= 2.f;
      const float sn = sinf(al * u);
      s[q] = u + ib * (sn * sn);
    }
  }
  OUT* yb = y + (size_t)b * L * C + c;
#pragma unroll
  for (int r = 0; r < ACT_R; ++r) {
    const int t = t0 + r;
    if (t < L) {
      float acc = 0.f;
#pragma unroll
      for (int m = 0; m < 12; ++m) acc += fd[m] * s[2 * r + m];
      store_act<OUT>(yb + (size_t)t * C, acc);
    }
  }
}

// ---------------------------------------------------------------- implicit-GEMM conv
constexpr int BM = 64, BN = 64, KC = 32;
constexpr int LDS_ROW = KC + 8;   // bf16 per LDS row: 80 bytes (16-byte aligned, staggers the 32 rows a wave reads)
constexpr int MAX_TAPS = 11, MAX_HALO = 64;

__host__ __device__ constexpr int conv_lds_bytes(int ksz, int halo) { return ((BM + halo) + ksz * BN) * LDS_ROW * 2; }

__global__ __launch_bounds__(256) void conv_kernel(const bf16* __restrict__ x, const bf16* __restrict__ w,
                                                   const float* __restrict__ bias, const float* resid, float* out,
                                                   float* sum, float sum_scale, int sum_init, int L, int Cin,
                                                   int Cin_pad, int N, int ksz, int dil, int pad) {
  extern __shared__ __align__(16) char smem[];
  const int halo = (ksz - 1) * dil;
  const int HR = BM + halo;
  bf16* As = (bf16*)smem;                       // [HR][LDS_ROW]
  bf16* Ws = As + HR * LDS_ROW;                 // [ksz][BN][LDS_ROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN, b = blockIdx.z;
  const bf16* xb = x + (size_t)b * L * Cin;
  const int Kw = ksz * Cin_pad;                 // packed weight row length
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  for (int c0 = 0; c0 < Cin_pad; c0 += KC) {
    // input rows m0 - pad .. m0 + BM - 1 + halo - pad, columns c0 .. c0 + 31, in 4-element (8-byte) groups; zero outside
    for (int e = tid; e < HR * (KC / 4); e += 256) {
      const int r = e / (KC / 4), g = e % (KC / 4);
      const int gr = m0 - pad + r, ci = c0 + g * 4;
      uint2 v = make_uint2(0u, 0u);
      if (gr >= 0 && gr < L && ci < Cin) v = *(const uint2*)(xb + (size_t)gr * Cin + ci);
      *(uint2*)(As + r * LDS_ROW + g * 4) = v;
    }
    // weights [n][tap][c0 .. c0 + 31] (rows padded to Npad, C_in padded to Cin_pad with zeros at pack time)
    for (int e = tid; e < ksz * BN * (KC / 8); e += 256) {
      const int g = e % (KC / 8), rn = e / (KC / 8);
      const int n = rn % BN, tap = rn / BN;
      const uint4 v = *(const uint4*)(w + (size_t)(n0 + n) * Kw + (size_t)tap * Cin_pad + c0 + g * 8);
      *(uint4*)(Ws + (tap * BN + n) * LDS_ROW + g * 8) = v;
    }
    __syncthreads();
    for (int tap = 0; tap < ksz; ++tap) {
      const bf16* ap = As + (wm * 32 + (lane & 31) + tap * dil) * LDS_ROW + (lane >> 5) * 8;
      const bf16* bp = Ws + (tap * BN + wn * 32 + (lane & 31)) * LDS_ROW + (lane >> 5) * 8;
#pragma unroll
      for (int kk = 0; kk < KC; kk += 16) {
        const bf16x8 av = *(const bf16x8*)(ap + kk);
        const bf16x8 bv = *(const bf16x8*)(bp + kk);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // accumulator register r of lane l: row 8 (r / 4) + 4 (l / 32) + r % 4, column l % 32
  const int n = n0 + wn * 32 + (lane & 31);
  if (n >= N) return;
  const float bn = bias ? bias[n] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int t = m0 + wm * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
    if (t >= L) continue;
    const size_t i = ((size_t)b * L + t) * N + n;
    float v = acc[r] + bn;
    if (resid) v += resid[i];
    if (out) out[i] = v;
    if (sum) sum[i] = sum_init ? v * sum_scale : sum[i] + v * sum_scale;
  }
}

F5eDeviceOnce g_conv_lds_once;

// ---------------------------------------------------------------- conv_post
__global__ __launch_bounds__(256) void post_kernel(const float* __restrict__ a, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ out, int L, int C,
                                                   int ksz, int use_tanh) {
  const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (t >= L) return;
  const int pad = (ksz - 1) / 2;
  float acc = 0.f;
  for (int k = 0; k < ksz; ++k) {
    const int j = t + k - pad;
    if (j < 0 || j >= L) continue;
    const float* ar = a + ((size_t)b * L + j) * C;
    const float* wr = w + (size_t)k * C;
    // one partial sum per tap on four independent accumulators, as the formula reads (sum_k sum_c): a single serial chain
    // over all ksz * C products loses about two more bits than that (it missed the 4x-fp32-yardstick gate at C = 24)
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
    int c = 0;
    for (; c + 3 < C; c += 4) {
      p0 += ar[c] * wr[c];
      p1 += ar[c + 1] * wr[c + 1];
      p2 += ar[c + 2] * wr[c + 2];
      p3 += ar[c + 3] * wr[c + 3];
    }
    for (; c < C; ++c) p0 += ar[c] * wr[c];
    acc += (p0 + p1) + (p2 + p3);
  }
  if (bias) acc += bias[0];
  out[(size_t)b * L + t] = use_tanh ? tanhf(acc) : fminf(fmaxf(acc, -1.f), 1.f);
}

}  // namespace

extern "C" {

int f5e_bigvgan_act(hipStream_t st, const float* x, void* y, int out_f32, const float* alpha, const float* inv_beta,
                    const float* f_up, const float* f_dn, int B, int L, int C) {
  F5E_REQUIRE(x && y && alpha && inv_beta && f_up && f_dn, "bigvgan_act: null operand");
  F5E_REQUIRE(B > 0 && L > 0 && C > 0, "bigvgan_act: bad shape B=%d L=%d C=%d", B, L, C);
  const int chunks = (L + ACT_R - 1) / ACT_R;
  const long long total = (long long)B * chunks * C;
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (out_f32)
    hipLaunchKernelGGL(act_kernel<float>, dim3(grid), dim3(256), 0, st, x, (float*)y, alpha, inv_beta, f_up, f_dn, L, C,
                       chunks, total);
  else
    hipLaunchKernelGGL(act_kernel<bf16>, dim3(grid), dim3(256), 0, st, x, (bf16*)y, alpha, inv_beta, f_up, f_dn, L, C,
                       chunks, total);
  F5E_LAUNCH_CHECK("bigvgan_act");
  return F5E_OK;
}

int f5e_bigvgan_conv(hipStream_t st, const void* x, const void* w_packed, const float* bias, const float* resid, float* out,
                     float* sum, float sum_scale, int sum_init, int B, int L, int Cin, int Cin_pad, int N, int ksz,
                     int dil, int pad) {
  F5E_REQUIRE(x && w_packed && (out || sum), "bigvgan_conv: null operand");
  F5E_REQUIRE(B > 0 && L > 0 && N > 0 && Cin > 0 && Cin % 4 == 0, "bigvgan_conv: bad shape (Cin=%d must be a multiple of 4)",
              Cin);
  F5E_REQUIRE(Cin_pad % KC == 0 && Cin_pad >= Cin, "bigvgan_conv: Cin_pad=%d must be a multiple of %d and >= Cin", Cin_pad,
              KC);
  F5E_REQUIRE(ksz >= 1 && ksz <= MAX_TAPS && dil >= 1 && (ksz - 1) * dil <= MAX_HALO && pad >= 0 && pad <= (ksz - 1) * dil,
              "bigvgan_conv: unsupported taps %d / dilation %d / pad %d", ksz, dil, pad);
  const int lds = conv_lds_bytes(ksz, (ksz - 1) * dil);
  if (lds > 64 * 1024) F5E_OPT_IN_LDS(g_conv_lds_once, conv_kernel, conv_lds_bytes(MAX_TAPS, MAX_HALO));
  dim3 grid((L + BM - 1) / BM, (N + BN - 1) / BN, B);
  hipLaunchKernelGGL(conv_kernel, grid, dim3(256), lds, st, (const bf16*)x, (const bf16*)w_packed, bias, resid, out, sum,
                     sum_scale, sum_init, L, Cin, Cin_pad, N, ksz, dil, pad);
  F5E_LAUNCH_CHECK("bigvgan_conv");
  return F5E_OK;
}

int f5e_bigvgan_post(hipStream_t st, const float* a, const float* w, const float* bias, float* out, int B, int L, int C,
                     int ksz, int use_tanh) {
  F5E_REQUIRE(a && w && out, "bigvgan_post: null operand");
  F5E_REQUIRE(B > 0 && L > 0 && C > 0 && ksz >= 1 && ksz % 2 == 1, "bigvgan_post: bad shape");
  hipLaunchKernelGGL(post_kernel, dim3((L + 255) / 256, B), dim3(256), 0, st, a, w, bias, out, L, C, ksz, use_tanh);
  F5E_LAUNCH_CHECK("bigvgan_post");
  return F5E_OK;
}

}  // extern "C"
