// The WavLM-large upstream of the SIM metric (s3prl "wavlm_large" in the reference, eval/ecapa_tdnn.py:171-199), exact fp32,
// channels-last: what the encoder needs beyond f5e_gemm_f32 / f5e_layernorm and the biased attention of ppg_attention.hip.
//
//   f5e_wav_norm         row-wise waveform normalisation (F.layer_norm(wav, wav.shape)) + the frame count of every row
//   f5e_wavlm_conv0      Conv1d(1 -> C, k 10, stride 5) + LayerNorm(C) + GELU, [B][S] -> [B][T0][C] in one pass
//   f5e_layernorm_gelu   LayerNorm(C) + GELU after the strided-view GEMMs of conv layers 1-6
//   f5e_wavlm_posconv    x + GELU(grouped Conv1d(D, D, k 128, pad 64) + bias) on v_mfma_f32_16x16x4_f32
//   f5e_wavlm_gate       the per-query gate of the relative-position bias
//
// Nothing here allocates, synchronises or reads back.  Per-row lengths are DEVICE int32.
#include "f5e_common.h"

namespace {

__device__ __forceinline__ float block_sum_256(float v, float* red) {   // 256 threads; red: 4 floats of LDS
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- waveform normalisation -----------------------------------------------------------------------------------------------
// A row of 30 s is 480k samples: it is cut into chunks of WN_CHUNK samples, one workgroup each.  Launch 1 leaves (mean, M2
// about that mean) per chunk; launch 2 merges the chunks of its row in a fixed order (Chan's update, in double) and applies.
// A chunk's figures depend only on the row's valid samples, so a padded row gives the bits of its B = 1 run.
constexpr int WN_CHUNK = 4096;

struct ConvGeom {
  int n, k[8], s[8];
};

__global__ __launch_bounds__(256) void wav_stats_kernel(const float* __restrict__ wav, int ldw, const int* __restrict__ len,
                                                        float* __restrict__ partials, int S, int nch) {
  __shared__ float red[4];
  const int b = blockIdx.y, c0 = blockIdx.x * WN_CHUNK;
  const int L = len ? min(max(len[b], 0), S) : S;
  const int n = min(max(L - c0, 0), WN_CHUNK);
  const float* p = wav + (size_t)b * ldw + c0;
  float v[WN_CHUNK / 256], s = 0.f;
#pragma unroll
  for (int e = 0; e < WN_CHUNK / 256; ++e) {
    const int i = threadIdx.x + 256 * e;
    v[e] = i < n ? p[i] : 0.f;
    s += v[e];
  }
  const float tot = block_sum_256(s, red);
  const float mean = n > 0 ? tot / (float)n : 0.f;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < WN_CHUNK / 256; ++e) {
    const float d = v[e] - mean;
    if (threadIdx.x + 256 * e < n) q += d * d;
  }
  q = block_sum_256(q, red);
  if (threadIdx.x == 0) {
    partials[((size_t)b * nch + blockIdx.x) * 2] = mean;
    partials[((size_t)b * nch + blockIdx.x) * 2 + 1] = q;
  }
}

__global__ __launch_bounds__(256) void wav_apply_kernel(const float* __restrict__ wav, int ldw, const int* __restrict__ len,
                                                        const float* __restrict__ partials, float* __restrict__ out, int ldo,
                                                        int* __restrict__ frames, float* __restrict__ mask, int t_mask, int S,
                                                        int nch, ConvGeom cg, float eps) {
  const int b = blockIdx.y, c0 = blockIdx.x * WN_CHUNK;
  const int L = len ? min(max(len[b], 0), S) : S;
  const float* pr = partials + (size_t)b * nch * 2;
  double mean = 0.0;
  for (int c = 0; c < nch; ++c) {
    const int n = min(max(L - c * WN_CHUNK, 0), WN_CHUNK);
    mean += (double)n * (double)pr[2 * c];
  }
  mean = L > 0 ? mean / (double)L : 0.0;
  double m2 = 0.0;
  for (int c = 0; c < nch; ++c) {
    const int n = min(max(L - c * WN_CHUNK, 0), WN_CHUNK);
    const double d = (double)pr[2 * c] - mean;
    if (n > 0) m2 += (double)pr[2 * c + 1] + (double)n * d * d;
  }
  const float rstd = (float)(1.0 / sqrt((L > 0 ? m2 / (double)L : 0.0) + (double)eps));
  const float mu = (float)mean;
  int fr = L;
  for (int l = 0; l < cg.n; ++l) fr = fr >= cg.k[l] ? (fr - cg.k[l]) / cg.s[l] + 1 : 0;
  if (blockIdx.x == 0 && threadIdx.x == 0 && frames) frames[b] = fr;
  const float* p = wav + (size_t)b * ldw;
  float* o = out + (size_t)b * ldo;
#pragma unroll
  for (int e = 0; e < WN_CHUNK / 256; ++e) {
    const int i = c0 + threadIdx.x + 256 * e;
    if (i < S) o[i] = i < L ? (p[i] - mu) * rstd : 0.f;
    if (mask && i < t_mask) mask[(size_t)b * t_mask + i] = i < fr ? 1.f : 0.f;
  }
}

// ---- LayerNorm(C) + GELU(erf) of one frame held by a wave: lane l has channels l + 64 j ----------------------------------
template <int NJ>
__device__ __forceinline__ void ln_gelu_wave(const float (&v)[NJ], int lane, int C, const float* __restrict__ gamma,
                                             const float* __restrict__ beta, float eps, float* __restrict__ out) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (lane + 64 * j < C) s += v[j];
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float d = v[j] - mean;
    if (lane + 64 * j < C) q += d * d;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    if (c < C) out[c] = gelu_erf_f((v[j] - mean) * rstd * gamma[c] + beta[c]);
  }
}

// Layer 0 of the extractor.  A workgroup owns C0_FT output frames: their 5 C0_FT + 5 samples go through LDS once, every wave
// keeps its 10 taps of C / 64 channels per lane in registers and walks the frames; the output write (the only large stream)
// is 256 contiguous bytes per wave and j.
constexpr int C0_FT = 64, C0_K = 10, C0_S = 5;

template <int NJ>
__global__ __launch_bounds__(256) void conv0_kernel(const float* __restrict__ wav, int ldw, const float* __restrict__ w,
                                                    const float* __restrict__ bias, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ out,
                                                    long long out_bstride, int T0, int C, float eps) {
  __shared__ float xs[C0_FT * C0_S + C0_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y, t0 = blockIdx.x * C0_FT;
  const int nf = min(C0_FT, T0 - t0);
  const int ns = (nf - 1) * C0_S + C0_K;
  const float* src = wav + (size_t)b * ldw + (size_t)t0 * C0_S;
  for (int i = tid; i < ns; i += 256) xs[i] = src[i];
  float wr[NJ][C0_K], br[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = lane + 64 * j;
    br[j] = (bias && c < C) ? bias[c] : 0.f;
#pragma unroll
    for (int k = 0; k < C0_K; ++k) wr[j][k] = c < C ? w[(size_t)c * C0_K + k] : 0.f;
  }
  __syncthreads();
  for (int f = wave; f < nf; f += 4) {
    float v[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < C0_K; ++k) a += wr[j][k] * xs[f * C0_S + k];
      v[j] = a + br[j];
    }
    ln_gelu_wave<NJ>(v, lane, C, gamma, beta, eps, out + (size_t)b * out_bstride + (size_t)(t0 + f) * C);
  }
}

template <int NJ>
__global__ __launch_bounds__(256) void ln_gelu_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int ldo,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      long long rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = x + (size_t)row * ldx;
  float v[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) v[j] = lane + 64 * j < C ? p[lane + 64 * j] : 0.f;
  ln_gelu_wave<NJ>(v, lane, C, gamma, beta, eps, out + (size_t)row * ldo);
}

// ---- positional convolution -----------------------------------------------------------------------------------------------
// Per group a GEMM  out[t][oc] = sum_{tap, ic} w[oc][ic][tap] x[t + tap - pad][ic]  with K = taps * cg.  One wave owns 16
// output channels of one group and PC_NT * 16 frames, no LDS: A = weights (m = oc), B = frames (n = t), so the accumulator of a
// lane is 4 consecutive channels of one frame (a 16-byte store).  The k index is permuted as in ppg_attention.hip: a lane's
// float4 covers ic = 16 j + 4 g + 0..3 on both operands and element r feeds k-slot g of step (j, r).
// PC_NT = 8 (128 frames per wave): the folded weights are read ceil(T / 128) times per batch row -- 4 times for 10 s of
// audio -- while the [128 + taps][cg] window of x that a wave re-reads per tap stays in its CU's L1.
constexpr int PC_NT = 8;

__global__ __launch_bounds__(64) void posconv_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ wp,
                                                     const float* __restrict__ bias, const int* __restrict__ frames,
                                                     float* __restrict__ out, int ldo, int T, int D, int G, int taps, int pad) {
  const int lane = threadIdx.x, c16 = lane & 15, g4 = lane >> 4;
  const int cg = D / G, OT = (cg + 15) / 16, NJ = OT;
  const int grp = blockIdx.y / OT, ot = blockIdx.y - grp * OT, b = blockIdx.z;
  const int t0 = blockIdx.x * (16 * PC_NT);
  const int len = frames ? min(max(frames[b], 0), T) : T;
  const int nt = min(PC_NT, (T - t0 + 15) / 16);
  const int oc_l = ot * 16 + c16;
  const bool a_row = oc_l < cg;
  const size_t row0 = (size_t)b * T;
  f32x4 acc[PC_NT];
#pragma unroll
  for (int i = 0; i < PC_NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // taps that reach a frame in [0, len) from this tile: t0 + tap - pad < len  and  t0 + 16 nt - 1 + tap - pad >= 0
  const int tap_lo = max(0, pad - (t0 + 16 * nt - 1)), tap_hi = min(taps, len - t0 + pad);
  for (int tap = tap_lo; tap < tap_hi; ++tap) {
    for (int j = 0; j < NJ; ++j) {
      const int ic = 16 * j + 4 * g4;
      const bool k_ok = ic < cg;                      // cg % 4 == 0: a float4 is wholly inside or outside the group
      f32x4 af = {0.f, 0.f, 0.f, 0.f};
      if (a_row && k_ok) af = *(const f32x4*)(wp + (((size_t)grp * taps + tap) * cg + oc_l) * cg + ic);
      const int ch = grp * cg + (k_ok ? ic : 0);
#pragma unroll
      for (int i = 0; i < PC_NT; ++i) {
        if (i < nt) {
          const int fr = t0 + 16 * i + c16 + tap - pad;
          const bool ok = k_ok && fr >= 0 && fr < len;
          const int frc = min(max(fr, 0), T - 1);
          f32x4 xf = *(const f32x4*)(x + (row0 + frc) * ldx + ch);
          if (!ok) xf = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[r], xf[r], acc[i], 0, 0, 0);
        }
      }
    }
  }
  const int oc4 = ot * 16 + 4 * g4;                  // this lane's 4 channels inside the group
  if (oc4 >= cg) return;
  const int ch = grp * cg + oc4;
  const f32x4 bv = *(const f32x4*)(bias + ch);
#pragma unroll
  for (int i = 0; i < PC_NT; ++i) {
    const int t = t0 + 16 * i + c16;
    if (i < nt && t < T) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (t < len) {
        const f32x4 xv = *(const f32x4*)(x + (row0 + t) * ldx + ch);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = xv[r] + gelu_erf_f(acc[i][r] + bv[r]);
      }
      *(f32x4*)(out + (row0 + t) * ldo + ch) = o;
    }
  }
}

// ---- gate of the relative-position bias ------------------------------------------------------------------------------------
constexpr int GATE_DK_MAX = 128;

__global__ __launch_bounds__(256) void gate_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ wg,
                                                   const float* __restrict__ bg, const float* __restrict__ cst,
                                                   float* __restrict__ gate, long long n, int T, int H, int dk) {
  __shared__ float ws[8 * GATE_DK_MAX + 8];
  for (int i = threadIdx.x; i < 8 * dk; i += 256) ws[i] = wg[i];
  if (threadIdx.x < 8) ws[8 * dk + threadIdx.x] = bg[threadIdx.x];
  __syncthreads();
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int h = (int)(idx % H);
  const long long row = idx / H;
  const float* xp = x + (size_t)row * ldx + h * dk;
  float p[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) p[o] = 0.f;
  for (int d = 0; d < dk; d += 4) {
    const f32x4 xv = *(const f32x4*)(xp + d);
#pragma unroll
    for (int o = 0; o < 8; ++o)
#pragma unroll
      for (int e = 0; e < 4; ++e) p[o] += ws[o * dk + d + e] * xv[e];
  }
#pragma unroll
  for (int o = 0; o < 8; ++o) p[o] += ws[8 * dk + o];
  const float a = 1.0f / (1.0f + expf(-((p[0] + p[1]) + (p[2] + p[3]))));
  const float bb = 1.0f / (1.0f + expf(-((p[4] + p[5]) + (p[6] + p[7]))));
  const long long bi = row / T;
  const int t = (int)(row - bi * T);
  gate[((size_t)bi * H + h) * T + t] = a * (bb * cst[h] - 1.0f) + 2.0f;
}

}  // namespace

extern "C" int f5e_wav_norm(hipStream_t st, const float* wav, int ldw, const int* len, float* out, int ldo, float* partials,
                            int* frames, float* mask, int t_mask, const int* conv_kernels_host, const int* conv_strides_host,
                            int n_conv, int B, int S) {
  F5E_REQUIRE(wav && out && partials, "wav_norm: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && S > 0 && ldw >= S && ldo >= S, "wav_norm: bad shape (B=%d S=%d ldw=%d ldo=%d)", B, S, ldw,
              ldo);
  F5E_REQUIRE(n_conv >= 0 && n_conv <= 8 && (n_conv == 0 || (conv_kernels_host && conv_strides_host)),
              "wav_norm: at most 8 conv layers, with their kernel sizes and strides (n_conv=%d)", n_conv);
  F5E_REQUIRE(!mask || (t_mask > 0 && t_mask <= S), "wav_norm: mask needs 0 < t_mask <= S (t_mask=%d)", t_mask);
  ConvGeom cg{};
  cg.n = n_conv;
  for (int l = 0; l < n_conv; ++l) {
    cg.k[l] = conv_kernels_host[l], cg.s[l] = conv_strides_host[l];
    F5E_REQUIRE(cg.k[l] > 0 && cg.s[l] > 0, "wav_norm: conv layer %d has kernel %d, stride %d", l, cg.k[l], cg.s[l]);
  }
  const int nch = (S + WN_CHUNK - 1) / WN_CHUNK;
  const dim3 grid((unsigned)nch, (unsigned)B);
  hipLaunchKernelGGL(wav_stats_kernel, grid, dim3(256), 0, st, wav, ldw, len, partials, S, nch);
  hipLaunchKernelGGL(wav_apply_kernel, grid, dim3(256), 0, st, wav, ldw, len, partials, out, ldo, frames, mask, t_mask, S, nch,
                     cg, 1e-5f);
  F5E_LAUNCH_CHECK("wav_norm");
  return F5E_OK;
}

extern "C" int f5e_wav_norm_partials(int B, int S, unsigned long long* floats_out_host) {
  F5E_REQUIRE(B > 0 && S > 0 && floats_out_host, "wav_norm_partials: bad arguments");
  *floats_out_host = 2ull * (unsigned long long)B * (unsigned long long)((S + WN_CHUNK - 1) / WN_CHUNK);
  return F5E_OK;
}

extern "C" int f5e_wavlm_conv0(hipStream_t st, const float* wav, int ldw, const float* w, const float* bias, const float* gamma,
                               const float* beta, float* out, long long out_bstride, int B, int S, int T0, int C) {
  F5E_REQUIRE(wav && w && gamma && beta && out, "wavlm_conv0: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && C > 0 && C <= 512, "wavlm_conv0: bad shape (B=%d C=%d; C <= 512)", B, C);
  F5E_REQUIRE(T0 > 0 && S >= C0_K && T0 <= (S - C0_K) / C0_S + 1 && ldw >= S,
              "wavlm_conv0: %d frames need %d samples (S=%d ldw=%d)", T0, (T0 - 1) * C0_S + C0_K, S, ldw);
  F5E_REQUIRE(out_bstride >= (long long)T0 * C, "wavlm_conv0: the batch stride of out must cover T0 * C floats");
  const dim3 grid((unsigned)((T0 + C0_FT - 1) / C0_FT), (unsigned)B);
#define GO(NJ) hipLaunchKernelGGL(conv0_kernel<NJ>, grid, dim3(256), 0, st, wav, ldw, w, bias, gamma, beta, out, out_bstride, T0, C, 1e-5f)
  if (C <= 64) GO(1);
  else if (C <= 128) GO(2);
  else if (C <= 256) GO(4);
  else GO(8);
#undef GO
  F5E_LAUNCH_CHECK("wavlm_conv0");
  return F5E_OK;
}

extern "C" int f5e_layernorm_gelu(hipStream_t st, const float* x, int ldx, float* out, int ldo, const float* gamma,
                                  const float* beta, long long rows, int C, float eps) {
  F5E_REQUIRE(x && out && gamma && beta, "layernorm_gelu: null operand");
  F5E_REQUIRE(rows > 0 && rows <= 4ll * 0x7fffffff && C > 0 && C <= 1024 && ldx >= C && ldo >= C,
              "layernorm_gelu: bad shape (rows=%lld C=%d ldx=%d ldo=%d; C <= 1024)", rows, C, ldx, ldo);
  const dim3 grid((unsigned)((rows + 3) / 4));
#define GO(NJ) hipLaunchKernelGGL(ln_gelu_kernel<NJ>, grid, dim3(256), 0, st, x, ldx, out, ldo, gamma, beta, rows, C, eps)
  if (C <= 64) GO(1);
  else if (C <= 128) GO(2);
  else if (C <= 256) GO(4);
  else if (C <= 512) GO(8);
  else GO(16);
#undef GO
  F5E_LAUNCH_CHECK("layernorm_gelu");
  return F5E_OK;
}

extern "C" int f5e_wavlm_posconv(hipStream_t st, const float* x, int ldx, const float* w_packed, const float* bias,
                                 const int* frames, float* out, int ldo, int B, int T, int D, int groups, int taps, int pad) {
  F5E_REQUIRE(x && w_packed && bias && out && x != out, "wavlm_posconv: null operand, or out aliases x");
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && D > 0 && groups > 0 && D % groups == 0 && (D / groups) % 4 == 0 && taps > 0 &&
                  pad >= 0 && pad < taps,
              "wavlm_posconv: bad shape (B=%d T=%d D=%d groups=%d taps=%d pad=%d; D / groups must be a multiple of 4)", B, T, D,
              groups, taps, pad);
  F5E_REQUIRE(ldx >= D && ldo >= D && ldx % 4 == 0 && ldo % 4 == 0, "wavlm_posconv: row strides must cover D and be multiples of 4");
  F5E_REQUIRE((((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)bias | (uintptr_t)out) & 15) == 0,
              "wavlm_posconv: x, w_packed, bias and out must be 16-byte aligned");
  const int cg = D / groups, OT = (cg + 15) / 16;
  F5E_REQUIRE((long long)groups * OT <= 65535, "wavlm_posconv: too many channel tiles");
  const dim3 grid((unsigned)((T + 16 * PC_NT - 1) / (16 * PC_NT)), (unsigned)(groups * OT), (unsigned)B);
  hipLaunchKernelGGL(posconv_kernel, grid, dim3(64), 0, st, x, ldx, w_packed, bias, frames, out, ldo, T, D, groups, taps, pad);
  F5E_LAUNCH_CHECK("wavlm_posconv");
  return F5E_OK;
}

extern "C" int f5e_wavlm_gate(hipStream_t st, const float* x, int ldx, const float* w_gate, const float* b_gate,
                              const float* head_const, float* gate, int B, int T, int H, int dk) {
  F5E_REQUIRE(x && w_gate && b_gate && head_const && gate, "wavlm_gate: null operand");
  F5E_REQUIRE(B > 0 && T > 0 && H > 0 && dk > 0 && dk % 4 == 0 && dk <= GATE_DK_MAX,
              "wavlm_gate: bad shape (B=%d T=%d H=%d dk=%d; dk a multiple of 4, at most %d)", B, T, H, dk, GATE_DK_MAX);
  F5E_REQUIRE(ldx >= H * dk && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0,
              "wavlm_gate: x needs a row stride >= H dk that is a multiple of 4, and a 16-byte aligned base");
  const long long n = (long long)B * T * H;
  F5E_REQUIRE((n + 255) / 256 <= 0x7fffffff, "wavlm_gate: too many rows");
  hipLaunchKernelGGL(gate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, ldx, w_gate, b_gate, head_const, gate,
                     n, T, H, dk);
  F5E_LAUNCH_CHECK("wavlm_gate");
  return F5E_OK;
}
