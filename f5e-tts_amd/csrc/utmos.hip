// The UTMOS predictor (utmos22_strong in the reference, eval/eval_utmos.py), exact fp32, channels-last: what it needs beyond the
// encoder ops shared with WavLM and Whisper (f5e_gemm_f32, f5e_layernorm, f5e_wavlm_posconv, f5e_mha_f32).
//
//   f5e_w2v_conv0_gn   Conv1d(1 -> C, k 10, stride 5) + GroupNorm(C groups: every channel over TIME) + GELU, two phases
//   f5e_lstm_f32       the recurrence of a uni- / bidirectional single-layer LSTM, ONE launch per time step
//   f5e_score_mean     per-frame score (a dot product with the last linear's weight) and its masked mean per utterance
//
// Nothing here allocates, synchronises or reads back.  Per-row lengths are DEVICE int32.  No floating-point atomics: every
// reduction runs in a fixed order, so a graph replay gives the bits of the eager run.
#include "f5e_common.h"

namespace {

// ---- layer 0 of the group-norm extractor ------------------------------------------------------------------------------------
// A channel is normalised over the T0_b frames of its own row, so the statistics need a pass over all of them before any output
// exists.  The 10-tap convolution is cheaper to recompute than to store: phase 1 leaves (mean, M2 about that mean) per chunk of
// GN_CHUNK frames and channel (the count of a chunk follows from T0_b), phase 2 merges the chunks of its row in a fixed order
// with the pairwise update of Chan et al. (in double; never E[x^2] - mean^2), recomputes the convolution and applies.
// A workgroup owns GN_CHUNK frames of 64 channels: lane = channel, the four waves interleave the frames.
constexpr int GN_CHUNK = 256, GN_K = 10, GN_S = 5;

struct ConvGeom {
  int n, k[8], s[8];
};

__device__ __forceinline__ float conv10(const float (&w)[GN_K], float bias, const float* xs) {
  float a = 0.f;
#pragma unroll
  for (int k = 0; k < GN_K; ++k) a += w[k] * xs[k];
  return a + bias;
}

__device__ __forceinline__ int gn_frames(const int* len, int b, int S) {   // T0_b
  const int L = len ? min(max(len[b], 0), S) : S;
  return L >= GN_K ? (L - GN_K) / GN_S + 1 : 0;
}

__device__ __forceinline__ float sum4_lds(float v, float (*red)[64], int wave, int lane) {   // fixed order over the 4 waves
  __syncthreads();
  red[wave][lane] = v;
  __syncthreads();
  return (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ __launch_bounds__(256) void gn_stats_kernel(const float* __restrict__ wav, int ldw, const float* __restrict__ w,
                                                       const float* __restrict__ bias, const int* __restrict__ len,
                                                       float* __restrict__ partials, int S, int C, int nch) {
  __shared__ float xs[GN_CHUNK * GN_S + GN_K];
  __shared__ float red[4][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, c = blockIdx.y * 64 + lane, t0 = blockIdx.x * GN_CHUNK;
  const int nf = min(max(gn_frames(len, b, S) - t0, 0), GN_CHUNK);
  if (nf == 0) return;                                    // the merge of phase 2 never reads an empty chunk
  const int ns = (nf - 1) * GN_S + GN_K;
  const float* src = wav + (size_t)b * ldw + (size_t)t0 * GN_S;
  for (int i = tid; i < ns; i += 256) xs[i] = src[i];
  float wr[GN_K];
#pragma unroll
  for (int k = 0; k < GN_K; ++k) wr[k] = c < C ? w[(size_t)c * GN_K + k] : 0.f;
  const float br = (bias && c < C) ? bias[c] : 0.f;
  __syncthreads();
  float s = 0.f;
  for (int f = wave; f < nf; f += 4) s += conv10(wr, br, xs + f * GN_S);
  const float mean = sum4_lds(s, red, wave, lane) / (float)nf;
  float q = 0.f;
  for (int f = wave; f < nf; f += 4) {
    const float d = conv10(wr, br, xs + f * GN_S) - mean;
    q += d * d;
  }
  q = sum4_lds(q, red, wave, lane);
  if (wave == 0 && c < C) {
    float* p = partials + (((size_t)b * nch + blockIdx.x) * C + c) * 2;
    p[0] = mean, p[1] = q;
  }
}

__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ wav, int ldw, const float* __restrict__ w,
                                                       const float* __restrict__ bias, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const int* __restrict__ len,
                                                       const float* __restrict__ partials, float* __restrict__ out,
                                                       long long out_bstride, int* __restrict__ frames,
                                                       float* __restrict__ mask, int t_mask, int S, int T0, int C, int nch,
                                                       ConvGeom cg, float eps) {
  __shared__ float xs[GN_CHUNK * GN_S + GN_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, c = blockIdx.y * 64 + lane, t0 = blockIdx.x * GN_CHUNK;
  const int L = len ? min(max(len[b], 0), S) : S;
  const int Tb = gn_frames(len, b, S);
  if (blockIdx.x == 0 && blockIdx.y == 0) {               // the frame count after every conv layer, and the frame mask
    int fr = L;
    for (int l = 0; l < cg.n; ++l) fr = fr >= cg.k[l] ? (fr - cg.k[l]) / cg.s[l] + 1 : 0;
    if (tid == 0 && frames) frames[b] = fr;
    if (mask)
      for (int i = tid; i < t_mask; i += 256) mask[(size_t)b * t_mask + i] = i < fr ? 1.f : 0.f;
  }
  const int nt = min(T0 - t0, GN_CHUNK);                  // frames this workgroup writes
  const int nf = min(max(Tb - t0, 0), nt);                // ... of which valid
  if (nf > 0) {
    const int ns = (nf - 1) * GN_S + GN_K;
    const float* src = wav + (size_t)b * ldw + (size_t)t0 * GN_S;
    for (int i = tid; i < ns; i += 256) xs[i] = src[i];
  }
  __syncthreads();
  if (c >= C) return;
  float* o = out + (size_t)b * out_bstride + (size_t)t0 * C + c;
  if (nf > 0) {
    double n = 0.0, mean = 0.0, m2 = 0.0;                 // Chan's pairwise update, chunk by chunk in ascending order
    for (int ch = 0; ch < nch; ++ch) {
      const int nb = min(max(Tb - ch * GN_CHUNK, 0), GN_CHUNK);
      if (nb == 0) break;
      const float* p = partials + (((size_t)b * nch + ch) * C + c) * 2;
      const double mb = (double)p[0], qb = (double)p[1];
      if (ch == 0) {
        n = (double)nb, mean = mb, m2 = qb;
      } else {
        const double tot = n + (double)nb, d = mb - mean;
        mean += d * ((double)nb / tot);
        m2 += qb + d * d * (n * (double)nb / tot);
        n = tot;
      }
    }
    const float mu = (float)mean;
    const float rstd = (float)(1.0 / sqrt(m2 / n + (double)eps));
    float wr[GN_K];
#pragma unroll
    for (int k = 0; k < GN_K; ++k) wr[k] = w[(size_t)c * GN_K + k];
    const float br = bias ? bias[c] : 0.f, g = gamma[c], be = beta[c];
    for (int f = wave; f < nf; f += 4)
      o[(size_t)f * C] = gelu_erf_f((conv10(wr, br, xs + f * GN_S) - mu) * rstd * g + be);
  }
  for (int f = nf + wave; f < nt; f += 4) o[(size_t)f * C] = 0.f;
}

// ---- LSTM recurrence --------------------------------------------------------------------------------------------------------
// One launch per time step; workgroup (x, dir) owns LSTM_UW hidden units of one direction with all four gate rows of each, one
// wave per unit.  Lane l holds k = l, l + 64, ...; w_hh is packed [dir][unit][k / 64][lane][gate] so that a lane's four gate
// weights of one k are one 16-byte load and a wave reads 1 KiB per instruction.  h of the neighbouring step comes straight from
// `out`, which the previous launch wrote (the launch boundary is the only ordering there is); the cell state of a unit has this
// one wave as its only reader and writer.  The grid and the workgroup -> slice mapping are the same at every step, so a slice
// is re-read from the L2 of the XCD that fetched it first (4 LSTM_UW H floats per workgroup: 32 KiB at H = 512).
// Packed-sequence semantics: step s is t = s for direction 0 and t = len_b - 1 - s for direction 1, for rows with s < len_b; a
// row at or beyond its length gets out[b][s] = 0 for this workgroup's units and reads nothing.
constexpr int LSTM_UW = 4;

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int BT>
__global__ __launch_bounds__(64 * LSTM_UW) void lstm_step_kernel(const float* __restrict__ xg, long long ldxg,
                                                                 const float* __restrict__ whh, const int* __restrict__ len,
                                                                 float* __restrict__ out, float* __restrict__ cell, int B,
                                                                 int T, int H, int ND, int step) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dir = blockIdx.y, u = blockIdx.x * LSTM_UW + wave;
  const int NJ = H >> 6, ldo = ND * H;
  const f32x4* wp = (const f32x4*)whh + ((size_t)dir * H + u) * H + lane;
  for (int b0 = 0; b0 < B; b0 += BT) {
    int t[BT];
    const float* hp[BT];
    f32x4 acc[BT], xv[BT];
#pragma unroll
    for (int i = 0; i < BT; ++i) {
      const int b = b0 + i;
      const int L = b < B ? (len ? min(max(len[b], 0), T) : T) : 0;
      t[i] = step < L ? (dir == 0 ? step : L - 1 - step) : -1;
      // h of the step before: t - 1 (forward) or t + 1 (backward); none at step 0
      hp[i] = (t[i] >= 0 && step > 0) ? out + ((size_t)b * T + (dir == 0 ? t[i] - 1 : t[i] + 1)) * ldo + (size_t)dir * H + lane
                                      : nullptr;
      acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      xv[i] = acc[i];
      if (t[i] >= 0) {                                    // issued before the dot products, used after them
        const float* xr = xg + ((size_t)b * T + t[i]) * ldxg + (size_t)dir * 4 * H + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) xv[i][g] = xr[(size_t)g * H];
      }
    }
    if (step > 0) {
#pragma unroll 4
      for (int j = 0; j < NJ; ++j) {                       // H / 64 independent 16-byte loads per lane: keep four in flight
        const f32x4 wv = wp[(size_t)j * 64];
#pragma unroll
        for (int i = 0; i < BT; ++i) {
          if (hp[i]) {
            const float h = hp[i][j * 64];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[i][g] += wv[g] * h;
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < BT; ++i) {
      const int b = b0 + i;
      if (b >= B) continue;                               // wave-uniform
      if (t[i] < 0) {
        if (lane == 0) out[((size_t)b * T + step) * ldo + (size_t)dir * H + u] = 0.f;
        continue;
      }
      float gsum[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) gsum[g] = wave_sum(acc[i][g]);
      if (lane == 0) {
        float* cp = cell + ((size_t)dir * B + b) * H + u;
        const float gi = sigmoid_f(xv[i][0] + gsum[0]), gf = sigmoid_f(xv[i][1] + gsum[1]);
        const float gg = tanhf(xv[i][2] + gsum[2]), go = sigmoid_f(xv[i][3] + gsum[3]);
        const float c = step > 0 ? gf * *cp + gi * gg : gi * gg;
        *cp = c;
        out[((size_t)b * T + t[i]) * ldo + (size_t)dir * H + u] = go * tanhf(c);
      }
    }
  }
}

// ---- score head ---------------------------------------------------------------------------------------------------------------
// One workgroup of SM_WAVES waves per batch row; wave w takes frames w, w + SM_WAVES, ... in ascending order and lane 0 keeps the
// wave's running sum; the SM_WAVES sums are added in ascending order.  A frame's dot product runs on four accumulators per lane
// (k = lane + 64 j, j mod 4), so four loads are in flight per operand; they are joined as (a0 + a1) + (a2 + a3).
constexpr int SM_WAVES = 16;

__global__ __launch_bounds__(64 * SM_WAVES) void score_mean_kernel(const float* __restrict__ hid, long long ldh,
                                                                   const float* __restrict__ w2, const float* __restrict__ b2,
                                                                   const int* __restrict__ frames,
                                                                   float* __restrict__ frame_scores, float* __restrict__ out,
                                                                   int T, int F, float scale, float offset) {
  __shared__ float red[SM_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
  const int n = frames ? min(max(frames[b], 0), T) : T;
  const float bias = b2 ? b2[0] : 0.f;
  float run = 0.f;
  for (int t = wave; t < T; t += SM_WAVES) {
    float s = 0.f;
    if (t < n) {
      const float* p = hid + ((size_t)b * T + t) * ldh;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      int k = lane;
      for (; k + 192 < F; k += 256) {
        a0 += p[k] * w2[k];
        a1 += p[k + 64] * w2[k + 64];
        a2 += p[k + 128] * w2[k + 128];
        a3 += p[k + 192] * w2[k + 192];
      }
      for (; k < F; k += 64) a0 += p[k] * w2[k];
      s = wave_sum((a0 + a1) + (a2 + a3)) + bias;
      run += s;
    }
    if (frame_scores && lane == 0) frame_scores[(size_t)b * T + t] = s;
  }
  if (lane == 0) red[wave] = run;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w) tot += red[w];
    out[b] = n > 0 ? scale * (tot / (float)n) + offset : offset;
  }
}

}  // namespace

extern "C" int f5e_w2v_conv0_gn_partials(int B, int S, int C, unsigned long long* floats_out_host) {
  F5E_REQUIRE(B > 0 && S >= GN_K && C > 0 && floats_out_host, "w2v_conv0_gn_partials: bad arguments (B=%d S=%d C=%d)", B, S, C);
  const int T0 = (S - GN_K) / GN_S + 1;
  *floats_out_host = 2ull * (unsigned long long)B * (unsigned long long)((T0 + GN_CHUNK - 1) / GN_CHUNK) * (unsigned long long)C;
  return F5E_OK;
}

extern "C" int f5e_w2v_conv0_gn(hipStream_t st, const float* wav, int ldw, const float* w, const float* bias,
                                const float* gamma, const float* beta, const int* len, float* partials, float* out,
                                long long out_bstride, int* frames, float* mask, int t_mask, const int* conv_kernels_host,
                                const int* conv_strides_host, int n_conv, int B, int S, int C, float eps) {
  F5E_REQUIRE(wav && w && gamma && beta && partials && out, "w2v_conv0_gn: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && C > 0 && C <= 64 * 65535 && S >= GN_K && ldw >= S,
              "w2v_conv0_gn: bad shape (B=%d S=%d ldw=%d C=%d; a row needs %d samples)", B, S, ldw, C, GN_K);
  const int T0 = (S - GN_K) / GN_S + 1;
  F5E_REQUIRE(out_bstride >= (long long)T0 * C, "w2v_conv0_gn: the batch stride of out must cover T0 * C = %lld floats",
              (long long)T0 * C);
  F5E_REQUIRE(n_conv >= 0 && n_conv <= 8 && (n_conv == 0 || (conv_kernels_host && conv_strides_host)),
              "w2v_conv0_gn: at most 8 conv layers, with their kernel sizes and strides (n_conv=%d)", n_conv);
  F5E_REQUIRE(!mask || (t_mask > 0 && t_mask <= S), "w2v_conv0_gn: mask needs 0 < t_mask <= S (t_mask=%d)", t_mask);
  F5E_REQUIRE(eps > 0.f, "w2v_conv0_gn: eps must be positive");
  ConvGeom cg{};
  cg.n = n_conv;
  for (int l = 0; l < n_conv; ++l) {
    cg.k[l] = conv_kernels_host[l], cg.s[l] = conv_strides_host[l];
    F5E_REQUIRE(cg.k[l] > 0 && cg.s[l] > 0, "w2v_conv0_gn: conv layer %d has kernel %d, stride %d", l, cg.k[l], cg.s[l]);
  }
  const int nch = (T0 + GN_CHUNK - 1) / GN_CHUNK;
  const dim3 grid((unsigned)nch, (unsigned)((C + 63) / 64), (unsigned)B);
  hipLaunchKernelGGL(gn_stats_kernel, grid, dim3(256), 0, st, wav, ldw, w, bias, len, partials, S, C, nch);
  hipLaunchKernelGGL(gn_apply_kernel, grid, dim3(256), 0, st, wav, ldw, w, bias, gamma, beta, len, partials, out, out_bstride,
                     frames, mask, t_mask, S, T0, C, nch, cg, eps);
  F5E_LAUNCH_CHECK("w2v_conv0_gn");
  return F5E_OK;
}

extern "C" int f5e_lstm_f32(hipStream_t st, const float* xg, long long ldxg, const float* w_hh_packed, const int* len,
                            float* out, float* cell, int B, int T, int H, int ND) {
  F5E_REQUIRE(xg && w_hh_packed && out && cell, "lstm_f32: null operand");
  F5E_REQUIRE(H >= 64 && H <= 1024 && H % 64 == 0, "lstm_f32: H = %d must be a multiple of 64, at most 1024", H);
  F5E_REQUIRE(B >= 1 && B <= 16 && (ND == 1 || ND == 2) && T >= 1 && T <= 4096,
              "lstm_f32: bad shape (B=%d T=%d ND=%d; B <= 16, ND 1 or 2, 1 <= T <= 4096)", B, T, ND);
  F5E_REQUIRE(ldxg >= (long long)ND * 4 * H, "lstm_f32: the row stride of xg (%lld) must cover ND * 4 H = %d floats", ldxg,
              ND * 4 * H);
  F5E_REQUIRE(((uintptr_t)w_hh_packed & 15) == 0, "lstm_f32: w_hh_packed must be 16-byte aligned");
  const dim3 grid((unsigned)(H / LSTM_UW), (unsigned)ND), block(64 * LSTM_UW);
  for (int s = 0; s < T; ++s) {
#define GO(BT) hipLaunchKernelGGL(lstm_step_kernel<BT>, grid, block, 0, st, xg, ldxg, w_hh_packed, len, out, cell, B, T, H, ND, s)
    if (B == 1) GO(1);
    else if (B == 2) GO(2);
    else GO(4);
#undef GO
  }
  F5E_LAUNCH_CHECK("lstm_f32");
  return F5E_OK;
}

extern "C" int f5e_score_mean(hipStream_t st, const float* hid, long long ldh, const float* w2, const float* b2,
                              const int* frames, float* frame_scores, float* out, int B, int T, int F, float scale,
                              float offset) {
  F5E_REQUIRE(hid && w2 && out, "score_mean: null operand");
  F5E_REQUIRE(B > 0 && T > 0 && F > 0 && ldh >= F, "score_mean: bad shape (B=%d T=%d F=%d ldh=%lld)", B, T, F, ldh);
  hipLaunchKernelGGL(score_mean_kernel, dim3((unsigned)B), dim3(64 * SM_WAVES), 0, st, hid, ldh, w2, b2, frames, frame_scores, out, T, F,
                     scale, offset);
  F5E_LAUNCH_CHECK("score_mean");
  return F5E_OK;
}
