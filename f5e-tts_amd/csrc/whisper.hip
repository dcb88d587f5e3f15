// Whisper on the device (reference infer/utils_infer.py:148-179, eval/utils_eval.py:631-672: openai/whisper-large-v3[-turbo]
// through transformers, greedy): the three parts that f5e_gemm_f32 / f5e_layernorm / f5e_mha_f32 / f5e_attn_decode_f32 /
// f5e_text_gather cannot express.  fp32 throughout.
//
//   f5e_whisper_logmel          WhisperFeatureExtractor: 400-point centred STFT (direct DFT against a twiddle table in LDS),
//                               Slaney mel, log10, the clamp at the utterance maximum - 8, (x + 4) / 4.  Two launches: the
//                               first leaves the raw log-mel and one maximum per workgroup, the second folds the maxima of its
//                               utterance in a fixed order and clamps in place.  No float atomics.
//   f5e_cross_attn_decode_f32   one query per (row, head) against encoder keys / values shared by the rows of an utterance.
//                               One workgroup of 4 waves per (row, head): wave w owns keys 64 w + 256 i + lane, keeps its own
//                               maximum, sum and context, and the four are merged through LDS with exp(m_w - M).
//   f5e_greedy_pick             suppression, first-maximum argmax and the token / done bookkeeping of one greedy step, so the
//                               token loop needs no host round trip per token.
//
// Nothing here allocates, synchronises or reads back.  Per-row lengths are DEVICE int32.
#include "f5e_common.h"

namespace {

// ---- log-mel front-end ----------------------------------------------------------------------------------------------------
// A workgroup owns LM_FT frames of one utterance.  Windowed frames, the twiddle table and the power spectrum live in LDS
// (LM_FT * 400 + 800 + LM_FT * 201 floats = 22.4 KB).  DFT: thread k < 201 owns bin k for all LM_FT frames -- the twiddle
// index k n mod 400 is carried incrementally, the frame samples are LDS broadcasts.  Mel: thread (m, g) owns filter m for the
// frames g, g + G, ...; the filterbank [201][n_mels] is read from global memory once per workgroup, coalesced over m.
constexpr int LM_NFFT = 400, LM_HOP = 160, LM_BINS = LM_NFFT / 2 + 1, LM_FT = 8;

__global__ __launch_bounds__(256) void logmel_kernel(const float* __restrict__ wav, int ldw, const int* __restrict__ len,
                                                     const float* __restrict__ window, const float* __restrict__ twiddle,
                                                     const float* __restrict__ fb, float* __restrict__ out,
                                                     float* __restrict__ partials, int T, int n_mels, int nwg) {
  __shared__ float xs[LM_FT][LM_NFFT];
  __shared__ float tc[LM_NFFT], ts[LM_NFFT];
  __shared__ float pw[LM_FT][LM_BINS + 3];
  __shared__ float red[4];
  const int tid = threadIdx.x, b = blockIdx.y, f0 = blockIdx.x * LM_FT;
  const int N = LM_HOP * T;                                   // the zero-padded row the extractor frames
  const int L = min(len ? min(max(len[b], 0), N) : N, ldw);   // samples at or beyond it count as zero
  const float* row = wav + (size_t)b * ldw;
  for (int i = tid; i < LM_NFFT; i += 256) tc[i] = twiddle[2 * i], ts[i] = twiddle[2 * i + 1];
  for (int e = tid; e < LM_FT * LM_NFFT; e += 256) {
    const int f = e / LM_NFFT, n = e - f * LM_NFFT;
    int i = (f0 + f) * LM_HOP - LM_NFFT / 2 + n;
    if (i < 0) i = -i;                                        // reflect, no edge repeat (N > n_fft / 2 is checked on the host)
    if (i >= N) i = 2 * (N - 1) - i;
    xs[f][n] = (f0 + f < T && i < L) ? row[i] * window[n] : 0.f;
  }
  __syncthreads();
  if (tid < LM_BINS) {
    float re[LM_FT], im[LM_FT];
#pragma unroll
    for (int f = 0; f < LM_FT; ++f) re[f] = 0.f, im[f] = 0.f;
    int idx = 0;
    for (int n = 0; n < LM_NFFT; ++n) {
      const float c = tc[idx], s = ts[idx];
#pragma unroll
      for (int f = 0; f < LM_FT; ++f) {
        const float x = xs[f][n];
        re[f] += x * c;
        im[f] += x * s;
      }
      idx += tid;
      if (idx >= LM_NFFT) idx -= LM_NFFT;
    }
#pragma unroll
    for (int f = 0; f < LM_FT; ++f) pw[f][tid] = re[f] * re[f] + im[f] * im[f];
  }
  __syncthreads();
  const int G = 256 / n_mels;                                 // 2 frame groups at 128 filters, 3 at 80
  const int m = tid % n_mels, g = tid / n_mels;
  float mx = -__builtin_inff();
  if (g < G) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};                      // LM_FT / 2 frames at the most
    for (int k = 0; k < LM_BINS; ++k) {
      const float w = fb[(size_t)k * n_mels + m];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int f = g + i * G;
        if (f < LM_FT) acc[i] += pw[f][k] * w;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = g + i * G;
      if (f < LM_FT && f0 + f < T) {
        const float v = log10f(fmaxf(acc[i], 1e-10f));
        out[((size_t)b * T + f0 + f) * n_mels + m] = v;
        mx = fmaxf(mx, v);
      }
    }
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) partials[(size_t)b * nwg + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void logmel_clamp_kernel(float* __restrict__ out, const float* __restrict__ partials, int T,
                                                           int n_mels, int nwg) {
  __shared__ float red[4];
  const int tid = threadIdx.x, b = blockIdx.y;
  float mx = -__builtin_inff();
  for (int i = tid; i < nwg; i += 256) mx = fmaxf(mx, partials[(size_t)b * nwg + i]);   // max is exact: the order is free
  mx = wave_max(mx);
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  const float floor_v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) - 8.0f;
  const size_t n = (size_t)LM_FT * n_mels, base = (size_t)b * T * n_mels + (size_t)blockIdx.x * n;
  const size_t end = (size_t)(b + 1) * T * n_mels;
  for (size_t e = base + tid; e < base + n && e < end; e += 256) out[e] = (fmaxf(out[e], floor_v) + 4.0f) / 4.0f;
}

// ---- single-query cross-attention --------------------------------------------------------------------------------------------
constexpr int XA_MAX_TK = 4096;

template <int DK>
__global__ __launch_bounds__(256) void cross_attn_decode_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ K,
                                                                int ldk, const float* __restrict__ V, int ldv,
                                                                float* __restrict__ out, int ldo, const int* __restrict__ kv_len,
                                                                int rows_per_utt, int Tk, float scale) {
  __shared__ float s[XA_MAX_TK];
  __shared__ float mrg[4][DK + 2];
  constexpr int G = DK >= 64 ? 1 : 64 / DK;     // key groups of a wave's context pass
  constexpr int DPL = DK > 64 ? DK / 64 : 1;    // channels per lane of the context pass
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int h = blockIdx.x, r = blockIdx.y, u = r / rows_per_utt;
  const int n = kv_len ? min(max(kv_len[u], 0), Tk) : Tk;
  const float* qr = q + (size_t)r * ldq + h * DK;
  const float* Ku = K + (size_t)u * Tk * ldk + h * DK;
  const float* Vu = V + (size_t)u * Tk * ldv + h * DK;
  f32x4 qv[DK / 4];
#pragma unroll
  for (int i = 0; i < DK / 4; ++i) qv[i] = *(const f32x4*)(qr + 4 * i);
  // ---- scores of this wave's keys
  float m = -__builtin_inff();
  for (int j = w * 64 + lane; j < n; j += 256) {
    const float* kr = Ku + (size_t)j * ldk;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < DK / 4; ++i) {
      const f32x4 kv = *(const f32x4*)(kr + 4 * i);
      acc += qv[i].x * kv.x + qv[i].y * kv.y + qv[i].z * kv.z + qv[i].w * kv.w;
    }
    acc *= scale;
    s[j] = acc;
    m = fmaxf(m, acc);
  }
  m = wave_max(m);
  float sum = 0.f;
  for (int j = w * 64 + lane; j < n; j += 256) {   // a lane rewrites only the entries it wrote
    const float e = expf(s[j] - m);
    s[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  __syncthreads();
  // ---- context of this wave's keys: lanes split as (key group, channel)
  const int g = DK >= 64 ? 0 : lane / DK, d0 = DK >= 64 ? lane : lane % DK;
  float acc[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) acc[i] = 0.f;
  for (int c = w * 64; c < n; c += 256) {
    const int hi = min(c + 64, n);
#pragma unroll 4
    for (int j = c + g; j < hi; j += G) {
      const float e = s[j];
      const float* vr = Vu + (size_t)j * ldv;
#pragma unroll
      for (int i = 0; i < DPL; ++i) acc[i] += e * vr[d0 + 64 * i];
    }
  }
#pragma unroll
  for (int o = 32; o >= DK; o >>= 1) acc[0] += __shfl_xor(acc[0], o, 64);   // fold the key groups (DK < 64 only)
  if (g == 0) {
#pragma unroll
    for (int i = 0; i < DPL; ++i) mrg[w][d0 + 64 * i] = acc[i];
  }
  if (lane == 0) mrg[w][DK] = m, mrg[w][DK + 1] = sum;
  __syncthreads();
  // ---- merge of the four waves
  if (tid < DK) {
    const float M = fmaxf(fmaxf(mrg[0][DK], mrg[1][DK]), fmaxf(mrg[2][DK], mrg[3][DK]));
    float o = 0.f, S = 0.f;
    if (M > -__builtin_inff()) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float f = expf(mrg[v][DK] - M);     // a wave without keys: exp(-inf) = 0
        S += mrg[v][DK + 1] * f;
        o += mrg[v][tid] * f;
      }
      o /= S;
    }
    out[(size_t)r * ldo + h * DK + tid] = o;      // no visible key: zeros
  }
}

// ---- greedy pick -----------------------------------------------------------------------------------------------------------------
constexpr int GP_MAX_V = 262144;   // one bit per class in LDS

__global__ __launch_bounds__(256) void greedy_pick_kernel(const float* __restrict__ logits, long long ld,
                                                          const int* __restrict__ suppress, int n_sup,
                                                          const int* __restrict__ begin_suppress, int n_beg, int* tokens,
                                                          int ld_tok, int* last, int* done, int V, int p, int eos) {
  __shared__ unsigned bits[GP_MAX_V / 32];
  __shared__ float rm[4];
  __shared__ int ra[4];
  const int tid = threadIdx.x, r = blockIdx.x;
  if (done[r]) {                                  // uniform over the workgroup
    if (tid == 0) tokens[(size_t)r * ld_tok + p + 1] = eos, last[r] = eos;
    return;
  }
  const int words = (V + 31) / 32;
  for (int i = tid; i < words; i += 256) bits[i] = 0u;
  __syncthreads();
  for (int i = tid; i < n_sup + n_beg; i += 256) {
    const int v = i < n_sup ? suppress[i] : begin_suppress[i - n_sup];
    if (v >= 0 && v < V) atomicOr(&bits[v >> 5], 1u << (v & 31));
  }
  __syncthreads();
  const float* row = logits + (size_t)r * ld;
  float m = -__builtin_inff();
  int arg = WAVE_NONE;
  for (int v = tid; v < V; v += 256) {            // ascending per thread: '>' keeps the first maximum; -inf takes the lowest index
    float x = row[v];
    if ((bits[v >> 5] >> (v & 31)) & 1u) x = -__builtin_inff();
    if (x > m || (arg == WAVE_NONE && !(x != x))) m = x, arg = v;
  }
  wave_argmax(m, arg);
  if ((tid & 63) == 0) rm[tid >> 6] = m, ra[tid >> 6] = arg;
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < 4; ++v)
      if (rm[v] > m || (rm[v] == m && ra[v] < arg)) m = rm[v], arg = ra[v];
    if (arg == WAVE_NONE) arg = 0;                // a row of NaN only
    tokens[(size_t)r * ld_tok + p + 1] = arg;
    last[r] = arg;
    if (arg == eos) done[r] = 1;
  }
}

__global__ __launch_bounds__(256) void alive_count_kernel(const int* __restrict__ done, int* __restrict__ alive, int R) {
  __shared__ int red[4];
  int c = 0;
  for (int r = threadIdx.x; r < R; r += 256) c += done[r] ? 0 : 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) *alive = (red[0] + red[1]) + (red[2] + red[3]);
}

}  // namespace

extern "C" int f5e_whisper_logmel_partials(int B, int T, unsigned long long* floats_out_host) {
  F5E_REQUIRE(B > 0 && T > 0 && floats_out_host, "whisper_logmel_partials: bad arguments");
  *floats_out_host = (unsigned long long)B * (unsigned long long)((T + LM_FT - 1) / LM_FT);
  return F5E_OK;
}

extern "C" int f5e_whisper_logmel(hipStream_t st, const float* wav, int ldw, const int* len, const float* window,
                                  const float* twiddle, const float* fb, float* out, float* partials, int B, int T, int n_fft,
                                  int hop, int n_mels) {
  F5E_REQUIRE(wav && window && twiddle && fb && out && partials, "whisper_logmel: null operand");
  if (n_fft != LM_NFFT || hop != LM_HOP || (n_mels != 80 && n_mels != 128)) {
    f5e_set_error("whisper_logmel: built for n_fft 400, hop 160 and 80 or 128 filters (got %d, %d, %d)", n_fft, hop, n_mels);
    return F5E_ERR_UNSUPPORTED;
  }
  F5E_REQUIRE(B > 0 && B <= 65535 && T >= 2 && T <= (1 << 22) && ldw > 0,
              "whisper_logmel: bad shape (B=%d T=%d ldw=%d; T >= 2 so that the reflection stays inside the row)", B, T, ldw);
  F5E_REQUIRE((long long)B * T * n_mels < (1ll << 40), "whisper_logmel: too large");
  const int nwg = (T + LM_FT - 1) / LM_FT;
  const dim3 grid((unsigned)nwg, (unsigned)B);
  hipLaunchKernelGGL(logmel_kernel, grid, dim3(256), 0, st, wav, ldw, len, window, twiddle, fb, out, partials, T, n_mels, nwg);
  hipLaunchKernelGGL(logmel_clamp_kernel, grid, dim3(256), 0, st, out, partials, T, n_mels, nwg);
  F5E_LAUNCH_CHECK("whisper_logmel");
  return F5E_OK;
}

extern "C" int f5e_cross_attn_decode_f32(hipStream_t st, const float* q, int ldq, const float* k, int ldk, const float* v,
                                         int ldv, float* out, int ldo, const int* kv_len, int R, int rows_per_utt, int Tk,
                                         int H, int dk, float scale) {
  F5E_REQUIRE(q && k && v && out, "cross_attn_decode_f32: null operand");
  F5E_REQUIRE(R > 0 && R <= 65535 && H > 0 && H <= 65535 && rows_per_utt > 0 && R % rows_per_utt == 0,
              "cross_attn_decode_f32: need 0 < R, H <= 65535 and R a multiple of rows_per_utt (R=%d rows_per_utt=%d)", R,
              rows_per_utt);
  if (dk != 16 && dk != 32 && dk != 64 && dk != 128) {
    f5e_set_error("cross_attn_decode_f32: head dim must be 16, 32, 64 or 128 (got %d)", dk);
    return F5E_ERR_UNSUPPORTED;
  }
  F5E_REQUIRE(Tk > 0 && Tk <= XA_MAX_TK, "cross_attn_decode_f32: need 0 < Tk <= %d", XA_MAX_TK);
  const long long HD = (long long)H * dk;
  F5E_REQUIRE(ldq >= HD && ldk >= HD && ldv >= HD && ldo >= HD, "cross_attn_decode_f32: a row stride is smaller than H * dk");
  F5E_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && (((uintptr_t)q | (uintptr_t)k) & 15) == 0,
              "cross_attn_decode_f32: q / k strides must be multiples of 4 floats, q and k 16-byte aligned");
  const dim3 grid((unsigned)H, (unsigned)R), block(256);
#define F5E_XA_LAUNCH(DK)                                                                                                   \
  hipLaunchKernelGGL(cross_attn_decode_kernel<DK>, grid, block, 0, st, q, ldq, k, ldk, v, ldv, out, ldo, kv_len, rows_per_utt, \
                     Tk, scale)
  switch (dk) {
    case 16: F5E_XA_LAUNCH(16); break;
    case 32: F5E_XA_LAUNCH(32); break;
    case 64: F5E_XA_LAUNCH(64); break;
    default: F5E_XA_LAUNCH(128); break;
  }
#undef F5E_XA_LAUNCH
  F5E_LAUNCH_CHECK("cross_attn_decode_f32");
  return F5E_OK;
}

extern "C" int f5e_greedy_pick(hipStream_t st, const float* logits, long long ld, const int* suppress, int n_sup,
                               const int* begin_suppress, int n_beg, int first_step, int* tokens, int ld_tok, int* last,
                               int* done, int* alive, int R, int V, int p, int eos) {
  F5E_REQUIRE(logits && tokens && last && done && alive, "greedy_pick: null operand");
  F5E_REQUIRE(R > 0 && R <= 0x7fffffff / 2 && V >= 1 && V <= GP_MAX_V && ld >= V,
              "greedy_pick: need R > 0, 1 <= V <= %d and ld >= V (R=%d V=%d)", GP_MAX_V, R, V);
  F5E_REQUIRE(n_sup >= 0 && n_beg >= 0 && (n_sup == 0 || suppress) && (n_beg == 0 || begin_suppress),
              "greedy_pick: a suppression list without its pointer");
  F5E_REQUIRE(p >= 0 && ld_tok >= p + 2, "greedy_pick: need p >= 0 and token rows of at least p + 2 columns");
  F5E_REQUIRE(eos >= 0 && eos < V, "greedy_pick: need 0 <= eos < V");
  hipLaunchKernelGGL(greedy_pick_kernel, dim3((unsigned)R), dim3(256), 0, st, logits, ld, suppress, n_sup, begin_suppress,
                     first_step ? n_beg : 0, tokens, ld_tok, last, done, V, p, eos);
  hipLaunchKernelGGL(alive_count_kernel, dim3(1), dim3(256), 0, st, done, alive, R);
  F5E_LAUNCH_CHECK("greedy_pick");
  return F5E_OK;
}
