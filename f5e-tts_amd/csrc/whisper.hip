// Whisper on the device (reference infer/utils_infer.py:148-179, eval/utils_eval.py:631-672: openai/whisper-large-v3[-turbo]
// through transformers, greedy or beam search): the parts that f5e_gemm_f32 / f5e_layernorm / f5e_mha_f32 / f5e_attn_decode_f32 /
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
//   f5e_whisper_beam_step       one step of the pooled beam search (transformers' generate(num_beams=K)): the logits go through
//                               LDS once, in chunks of 8192 classes that each leave a maximum, a sum of exponentials and their 2K
//                               largest unsuppressed classes; one workgroup per utterance then folds the chunks, takes the 2K
//                               largest candidates and applies the rules (open rows, pool of finished hypotheses, flags).
//   f5e_whisper_ts_pick         the greedy step under Whisper's timestamp rules (transformers' WhisperTimeStampLogitsProcessor):
//   f5e_whisper_ts_rule         one launch per step reads a row once, keeps a running log-sum-exp and argmax for the allowed
//   f5e_whisper_beam_step_ts    timestamps and for the allowed text apart, decides, picks and accumulates the pick's
//                               log-probability; the same pass without the pick leaves a rule descriptor per row that the beam
//                               step's chunk launch applies as one more mask.
//   f5e_whisper_sample_pick     f5e_whisper_ts_pick with a draw from softmax(x / T) over the allowed classes in place of the
//                               argmax (Gumbel-max; the noise is Philox4x32-10 of (class, step, serial, row key) and a seed).
//
// Nothing here allocates, synchronises or reads back.  Per-row lengths are DEVICE int32.
#include "f5e_common.h"
#include "whisper_pick.h"

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

// ---- the picks: the bodies (greedy_pick_step, ts_rule_step, ts_sample_step, alive_count_rows) are whisper_pick.h's, shared with
// the device-position kernels of whisper_step.hip --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void greedy_pick_kernel(const float* __restrict__ logits, long long ld,
                                                          const int* __restrict__ suppress, int n_sup,
                                                          const int* __restrict__ begin_suppress, int n_beg, int* tokens,
                                                          int ld_tok, int* last, int* done, int V, int p, int eos) {
  greedy_pick_step(logits, ld, suppress, n_sup, begin_suppress, n_beg, tokens, ld_tok, last, done, V, p, eos);
}

__global__ __launch_bounds__(256) void alive_count_kernel(const int* __restrict__ done, int* __restrict__ alive, int R) {
  __shared__ int red[4];
  const int n = alive_count_rows(done, R, red);
  if (threadIdx.x == 0) *alive = n;
}

template <bool PICK>
__global__ __launch_bounds__(256) void ts_rule_kernel(const float* __restrict__ logits, long long ld,
                                                      const int* __restrict__ suppress, int n_sup,
                                                      const int* __restrict__ begin_suppress, int n_beg, int* tokens, int ld_tok,
                                                      int* last, int* done, float* sum_logp, int* __restrict__ desc, int V, int p,
                                                      int n0, int eos, int no_ts, int max_initial) {
  ts_rule_step<PICK>(logits, ld, suppress, n_sup, begin_suppress, n_beg, tokens, ld_tok, last, done, sum_logp, desc, V, p, n0, eos,
                     no_ts, max_initial);
}

__global__ __launch_bounds__(256) void ts_sample_kernel(const float* __restrict__ logits, long long ld,
                                                        const int* __restrict__ suppress, int n_sup,
                                                        const int* __restrict__ begin_suppress, int n_beg, int* tokens, int ld_tok,
                                                        int* last, int* done, float* sum_logp, int V, int p, int n0, int eos,
                                                        int no_ts, int max_initial, float temperature, unsigned seed_lo,
                                                        unsigned seed_hi, const int* __restrict__ row_key,
                                                        const int* __restrict__ serial) {
  ts_sample_step(logits, ld, suppress, n_sup, begin_suppress, n_beg, tokens, ld_tok, last, done, sum_logp, V, p, n0, eos, no_ts,
                 max_initial, temperature, seed_lo, seed_hi, row_key, serial);
}

// ---- beam step (transformers' GenerationMixin._beam_search: K open rows, a pool of finished hypotheses) ------------------------
// Launch 1, one workgroup per (row, chunk of WB_CHUNK classes): the chunk goes from memory to LDS once (float4 when the row
// allows it); its maximum and sum of exponentials cover ALL its classes, then the suppressed ones become -inf and the 2K largest
// of what is left are taken by 2K rounds of (argmax over LDS, remove), lowest class first among equals.  Record per (row, chunk)
// in scratch: max, sum, 2K raw values (-inf: none), 2K classes (-1: none).  A row whose score is not above -inf has no finite
// candidate: its workgroups leave at once and launch 2 never reads its records.
// Launch 2, one workgroup per utterance: thread q folds the chunk maxima and sums of row q in ascending chunk order; the
// K * chunks * 2K survivors become (score + logp, row << 18 | class) in LDS (in the scratch itself beyond WB_LDS_CAND of them) and
// the 2K largest are taken by the same rounds, lowest (row, class) first among equals; one thread then applies the rules to at
// most 32 candidates, and all threads gather the tables and move the pool rows.
constexpr int WB_CHUNK = 8192, WB_MAX_K = 16, WB_MAX_V = 262144, WB_LDS_CAND = 4096, WB_NEW = 100;

__host__ __device__ inline int wb_chunks(int V) { return (V + WB_CHUNK - 1) / WB_CHUNK; }
__host__ __device__ inline int wb_rec(int K) { return 2 + 4 * K; }   // words of a (row, chunk) record

__global__ __launch_bounds__(256) void beam_chunk_kernel(const float* __restrict__ logits, long long ld,
                                                         const int* __restrict__ suppress, int n_sup,
                                                         const int* __restrict__ begin_suppress, int n_beg,
                                                         const float* __restrict__ score, float* __restrict__ scratch, int V,
                                                         int K, int vec, const int* __restrict__ desc, int eos, int no_ts) {
  __shared__ __attribute__((aligned(16))) float x[WB_CHUNK];
  __shared__ float rm[4];
  __shared__ int ra[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = blockIdx.y, r = blockIdx.x;
  const float NEG = -__builtin_inff();
  if (!(score[r] > NEG)) return;                                   // uniform over the workgroup
  const int c0 = c * WB_CHUNK, n = min(V - c0, WB_CHUNK), K2 = 2 * K;
  const float* row = logits + (size_t)r * ld + c0;
  float m = NEG;
  if (vec) {                                                       // ld % 4 == 0 and a 16-byte aligned base: c0 is a multiple of 4
    const int n4 = n >> 2;
    for (int i = tid; i < n4; i += 256) {
      const f32x4 v = *(const f32x4*)(row + 4 * i);
      *(f32x4*)(x + 4 * i) = v;
      m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    for (int i = 4 * n4 + tid; i < n; i += 256) x[i] = row[i], m = fmaxf(m, x[i]);
  } else {
    for (int i = tid; i < n; i += 256) x[i] = row[i], m = fmaxf(m, x[i]);
  }
  m = wave_max(m);
  if (lane == 0) rm[w] = m;
  __syncthreads();
  m = fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3]));
  float sum = 0.f;
  if (m > NEG)
    for (int i = tid; i < n; i += 256) sum += expf(x[i] - m);
  sum = wave_sum(sum);
  __syncthreads();                                                 // rm is reused; every x was read before a class is struck
  if (lane == 0) rm[w] = sum;
  for (int i = tid; i < n_sup + n_beg; i += 256) {
    const int v = (i < n_sup ? suppress[i] : begin_suppress[i - n_sup]) - c0;
    if (v >= 0 && v < n) x[v] = NEG;
  }
  if (desc) {                                                      // the row's timestamp rules (ts_rule_kernel): one more mask
    const int kind = desc[4 * r], lo = desc[4 * r + 1], hi = desc[4 * r + 2], ts_begin = no_ts + 1;
    const int text_from = kind == 2 ? ts_begin : kind == 1 ? eos : 0;
    for (int i = tid; i < n; i += 256) {
      const int v = c0 + i;
      if (v == no_ts || (v >= ts_begin ? (v < lo || v > hi) : v < text_from)) x[i] = NEG;
    }
  }
  __syncthreads();
  float* rec = scratch + ((size_t)r * gridDim.y + c) * wb_rec(K);
  if (tid == 0) rec[0] = m, rec[1] = (rm[0] + rm[1]) + (rm[2] + rm[3]);
  __syncthreads();
  for (int t = 0; t < K2; ++t) {
    float bm = NEG;
    int ba = WAVE_NONE;
    for (int i = tid; i < n; i += 256) {                           // ascending per thread: '>' keeps the first maximum
      const float v = x[i];
      if (v > bm) bm = v, ba = i;
    }
    wave_argmax(bm, ba);
    if (lane == 0) rm[w] = bm, ra[w] = ba;
    __syncthreads();
    bm = rm[0], ba = ra[0];
#pragma unroll
    for (int v = 1; v < 4; ++v)
      if (rm[v] > bm || (rm[v] == bm && ra[v] < ba)) bm = rm[v], ba = ra[v];
    const bool none = ba == WAVE_NONE || !(bm < __builtin_inff());  // nothing finite is left (uniform)
    if (tid == 0) {
      rec[2 + t] = none ? NEG : bm;
      ((int*)rec)[2 + K2 + t] = none ? -1 : c0 + ba;
      if (!none) x[ba] = NEG;
    }
    __syncthreads();
    if (none) {
      for (int u = t + 1 + tid; u < K2; u += 256) rec[2 + u] = NEG, ((int*)rec)[2 + K2 + u] = -1;
      break;
    }
  }
}

__global__ __launch_bounds__(256) void beam_select_kernel(float* score, const int* __restrict__ hyp_in,
                                                          const int* __restrict__ anc_in, int* __restrict__ hyp_out,
                                                          int* __restrict__ anc_out, int ld, int* __restrict__ last, int* pool_hyp,
                                                          int* pool_len, float* pool_score, int* pool_n, int* open_, int* alive,
                                                          float* scratch, int NCH, int K, int p, int n0, int cap, int eos,
                                                          float length_penalty) {
  __shared__ float cv_l[WB_LDS_CAND];
  __shared__ int ci_l[WB_LDS_CAND];
  __shared__ float row_sc[WB_MAX_K], row_m[WB_MAX_K], row_ls[WB_MAX_K];
  __shared__ float top_v[2 * WB_MAX_K], sel_val[WB_MAX_K], ps[WB_MAX_K];
  __shared__ int top_i[2 * WB_MAX_K], sel_par[WB_MAX_K], sel_cls[WB_MAX_K], pl[WB_MAX_K], pl_old[WB_MAX_K], src[WB_MAX_K];
  __shared__ float rm[4];
  __shared__ int ra[4], n_top, dirty;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, b = blockIdx.x;
  const float NEG = -__builtin_inff();
  const int K2 = 2 * K, REC = wb_rec(K), per_row = NCH * K2, N = K * per_row;
  const long long r0 = (long long)b * K;
  float* sb = scratch + (size_t)r0 * NCH * REC;                    // this utterance's records
  const bool in_lds = N <= WB_LDS_CAND;
  // candidate i = (row q, chunk c, rank j): where its value and id live
  auto slot = [&](int i) { const int rc = i / K2; return in_lds ? i : rc * REC + 2 + (i - rc * K2); };
  float* cv = in_lds ? cv_l : sb;
  int* ci = in_lds ? ci_l : (int*)sb + K2;
  if (tid < K) {
    const float sc = score[r0 + tid];
    float M = NEG, S = 0.f;
    if (sc > NEG) {
      const float* rr = sb + (size_t)tid * NCH * REC;
      for (int c = 0; c < NCH; ++c) M = fmaxf(M, rr[(size_t)c * REC]);
      for (int c = 0; c < NCH; ++c) {                              // ascending chunks: a fixed order
        const float mc = rr[(size_t)c * REC];
        if (mc > NEG) S += rr[(size_t)c * REC + 1] * expf(mc - M);
      }
    }
    row_sc[tid] = sc, row_m[tid] = M, row_ls[tid] = logf(S);
  }
  __syncthreads();
  for (int i = tid; i < N; i += 256) {
    const int q = i / per_row, rc = i / K2, j = i - rc * K2;
    float v = NEG;
    int id = WAVE_NONE;
    if (row_sc[q] > NEG) {
      const float xr = sb[(size_t)rc * REC + 2 + j];
      const int cls = ((const int*)sb)[(size_t)rc * REC + 2 + K2 + j];
      if (cls >= 0) {
        v = row_sc[q] + ((xr - row_m[q]) - row_ls[q]);
        id = (q << 18) | cls;
        if (!(v > NEG && v < __builtin_inff())) v = NEG;           // NaN and +inf are no candidates
      }
    }
    cv[slot(i)] = v, ci[slot(i)] = id;
  }
  if (tid == 0) n_top = K2;
  __syncthreads();
  for (int t = 0; t < K2; ++t) {
    float bm = NEG;
    int ba = WAVE_NONE, bi = -1;
    for (int i = tid; i < N; i += 256) {
      const float v = cv[slot(i)];
      const int id = ci[slot(i)];
      if (v > bm || (v == bm && v > NEG && id < ba)) bm = v, ba = id, bi = i;
    }
    const int mine = ba;
    wave_argmax(bm, ba);
    if (lane == 0) rm[w] = bm, ra[w] = ba;
    __syncthreads();
    bm = rm[0], ba = ra[0];
#pragma unroll
    for (int v = 1; v < 4; ++v)
      if (rm[v] > bm || (rm[v] == bm && ra[v] < ba)) bm = rm[v], ba = ra[v];
    const bool none = ba == WAVE_NONE;                              // uniform
    if (!none && mine == ba && bi >= 0) cv[slot(bi)] = NEG;         // ids are unique: one thread owns the winner
    if (tid == 0) {
      if (none) n_top = t;
      else top_v[t] = bm, top_i[t] = ba;
    }
    __syncthreads();
    if (none) break;
  }
  // ---- the rules, on at most 2K candidates in descending order
  if (tid == 0) {
    const int nc = n_top;
    int n = min(max(pool_n[b], 0), K), op = open_[b] != 0, n_run = 0, changed = 0;
    bool any_open_cand = false;
    for (int s = 0; s < K; ++s) ps[s] = pool_score[r0 + s], pl[s] = pl_old[s] = pool_len[r0 + s], src[s] = s;
    const float denom = powf((float)(p + 2 - n0), length_penalty);
    for (int j = 0; j < nc; ++j) {
      const int cls = top_i[j] & 0x3ffff;
      const bool hit = cls == eos || p + 2 >= cap;
      if (!hit) {
        any_open_cand = true;
        if (n_run < K) sel_par[n_run] = top_i[j] >> 18, sel_cls[n_run] = cls, sel_val[n_run] = top_v[j], ++n_run;
      } else if (op && j < K) {
        const float sc = top_v[j] / denom;
        int pos = n;
        while (pos > 0 && ps[pos - 1] < sc) --pos;                  // after every entry that is not worse
        if (pos < K) {
          for (int s = min(n, K - 1); s > pos; --s) ps[s] = ps[s - 1], pl[s] = pl[s - 1], src[s] = src[s - 1];
          ps[pos] = sc, pl[pos] = p + 2, src[pos] = WB_NEW + j;
          n = min(n + 1, K);
          changed = 1;
        }
      }
    }
    if (n == K) op = op && (n_run > 0 ? sel_val[0] / denom : NEG) > ps[K - 1];
    for (int q = n_run; q < K; ++q) sel_par[q] = q, sel_cls[q] = eos, sel_val[q] = NEG;
    for (int q = 0; q < K; ++q) score[r0 + q] = sel_val[q], last[r0 + q] = sel_cls[q];
    if (changed) {
      for (int s = 0; s < n; ++s)
        if (src[s] != s) pool_score[r0 + s] = ps[s], pool_len[r0 + s] = pl[s];
      pool_n[b] = n;
    }
    open_[b] = op;
    alive[b] = op && any_open_cand;
    dirty = changed ? n : 0;
  }
  __syncthreads();
  // ---- gather the parents' prefixes, append
  const int n_h = p + 2, n_a = p + 1;
  for (int i = tid; i < K * n_h; i += 256) {
    const int q = i / n_h, c = i % n_h;
    hyp_out[(r0 + q) * ld + c] = c == p + 1 ? sel_cls[q] : hyp_in[(r0 + sel_par[q]) * ld + c];
  }
  for (int i = tid; i < K * n_a; i += 256) {
    const int q = i / n_a, c = i % n_a;
    anc_out[(r0 + q) * ld + c] = c == p ? (int)r0 + sel_par[q] : anc_in[(r0 + sel_par[q]) * ld + c];
  }
  // ---- the pool's rows, from the last slot down: an old entry only moves to a higher slot, so its source is still whole
  for (int s = dirty - 1; s >= 0; --s) {
    const int from = src[s];
    if (from == s) continue;                                        // uniform
    int* dst = pool_hyp + (r0 + s) * ld;
    if (from >= WB_NEW) {
      const int id = top_i[from - WB_NEW];
      const int* par = hyp_in + (r0 + (id >> 18)) * ld;
      for (int c = tid; c < n_h; c += 256) dst[c] = c == p + 1 ? (id & 0x3ffff) : par[c];
    } else {
      const int* old = pool_hyp + (r0 + from) * ld;
      const int n_old = min(max(pl_old[from], 0), ld);               // the caller's lengths: kept inside the row
      for (int c = tid; c < n_old; c += 256) dst[c] = old[c];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int f5e_whisper_beam_scratch(int B, int K, int V, unsigned long long* bytes_out_host) {
  F5E_REQUIRE(B > 0 && B <= 65535 && K >= 1 && K <= WB_MAX_K && V >= 2 * K && V <= WB_MAX_V && bytes_out_host,
              "whisper_beam_scratch: need 0 < B <= 65535, 1 <= K <= %d, 2 K <= V <= %d (B=%d K=%d V=%d)", WB_MAX_K, WB_MAX_V, B, K,
              V);
  *bytes_out_host = (unsigned long long)B * K * wb_chunks(V) * wb_rec(K) * sizeof(float);
  return F5E_OK;
}

// desc == nullptr: the step without the timestamp rules.  Otherwise i32 [B*K][4], filled here by ts_rule_kernel from hyp_in.
static int beam_step_impl(hipStream_t st, const float* logits, long long ld_logits, const int* suppress, int n_sup,
                          const int* begin_suppress, int n_beg, float* score, const int* hyp_in, const int* anc_in, int* hyp_out,
                          int* anc_out, int ld, int* last, int* pool_hyp, int* pool_len, float* pool_score, int* pool_n, int* open,
                          int* alive, void* scratch, unsigned long long scratch_bytes, int B, int K, int V, int p, int n0, int cap,
                          int eos, float length_penalty, int* desc, int no_ts, int max_initial) {
  F5E_REQUIRE(logits && score && hyp_in && anc_in && hyp_out && anc_out && last && pool_hyp && pool_len && pool_score && pool_n &&
                  open && alive && scratch,
              "whisper_beam_step: null operand");
  F5E_REQUIRE(hyp_in != hyp_out && anc_in != anc_out, "whisper_beam_step: the hyp / anc tables are double-buffered (in != out)");
  if (K < 1 || K > WB_MAX_K || V > WB_MAX_V) {
    f5e_set_error("whisper_beam_step: built for 1 <= K <= %d and V <= %d (got K=%d V=%d)", WB_MAX_K, WB_MAX_V, K, V);
    return F5E_ERR_UNSUPPORTED;
  }
  F5E_REQUIRE(B > 0 && B <= 65535 && V >= 2 * K && ld_logits >= V,
              "whisper_beam_step: need 0 < B <= 65535, V >= 2 K and ld_logits >= V (B=%d K=%d V=%d)", B, K, V);
  F5E_REQUIRE(n_sup >= 0 && n_beg >= 0 && (n_sup == 0 || suppress) && (n_beg == 0 || begin_suppress),
              "whisper_beam_step: a suppression list without its pointer");
  F5E_REQUIRE(eos >= 0 && eos < V, "whisper_beam_step: need 0 <= eos < V");
  F5E_REQUIRE(n0 >= 1 && p >= n0 - 1 && ld >= p + 2 && cap <= ld,
              "whisper_beam_step: need n0 >= 1, p >= n0 - 1, tables of at least p + 2 columns and cap <= ld (n0=%d p=%d ld=%d "
              "cap=%d)", n0, p, ld, cap);
  const int NCH = wb_chunks(V);
  const unsigned long long need = (unsigned long long)B * K * NCH * wb_rec(K) * sizeof(float);
  F5E_REQUIRE(scratch_bytes >= need && ((uintptr_t)scratch & 3) == 0,
              "whisper_beam_step: scratch of %llu bytes, 4-byte aligned (f5e_whisper_beam_scratch); got %llu", need, scratch_bytes);
  const int vec = ld_logits % 4 == 0 && ((uintptr_t)logits & 15) == 0;
  if (desc)
    hipLaunchKernelGGL(ts_rule_kernel<false>, dim3((unsigned)(B * K)), dim3(256), 0, st, logits, ld_logits, suppress, n_sup,
                       begin_suppress, p + 1 == n0 ? n_beg : 0, const_cast<int*>(hyp_in), ld, nullptr, nullptr, nullptr, desc, V, p,
                       n0, eos, no_ts, max_initial);
  hipLaunchKernelGGL(beam_chunk_kernel, dim3((unsigned)(B * K), (unsigned)NCH), dim3(256), 0, st, logits, ld_logits, suppress,
                     n_sup, begin_suppress, p + 1 == n0 ? n_beg : 0, score, (float*)scratch, V, K, vec, desc, eos, no_ts);
  hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)B), dim3(256), 0, st, score, hyp_in, anc_in, hyp_out, anc_out, ld, last,
                     pool_hyp, pool_len, pool_score, pool_n, open, alive, (float*)scratch, NCH, K, p, n0, cap, eos,
                     length_penalty);
  F5E_LAUNCH_CHECK("whisper_beam_step");
  return F5E_OK;
}

extern "C" int f5e_whisper_beam_step(hipStream_t st, const float* logits, long long ld_logits, const int* suppress, int n_sup,
                                     const int* begin_suppress, int n_beg, float* score, const int* hyp_in, const int* anc_in,
                                     int* hyp_out, int* anc_out, int ld, int* last, int* pool_hyp, int* pool_len,
                                     float* pool_score, int* pool_n, int* open, int* alive, void* scratch,
                                     unsigned long long scratch_bytes, int B, int K, int V, int p, int n0, int cap, int eos,
                                     float length_penalty) {
  return beam_step_impl(st, logits, ld_logits, suppress, n_sup, begin_suppress, n_beg, score, hyp_in, anc_in, hyp_out, anc_out, ld,
                        last, pool_hyp, pool_len, pool_score, pool_n, open, alive, scratch, scratch_bytes, B, K, V, p, n0, cap, eos,
                        length_penalty, nullptr, 0, -1);
}

// The arguments every ruled entry shares: <|notimestamps|> is a class with at least one timestamp above it.
#define F5E_TS_REQUIRE(name)                                                                                                  \
  F5E_REQUIRE(no_timestamps >= 0 && no_timestamps + 1 < V && eos <= no_timestamps && max_initial >= -1,                        \
              name ": need 0 <= eos <= no_timestamps < V - 1 and max_initial >= -1 (eos=%d no_timestamps=%d V=%d "              \
                   "max_initial=%d)", eos, no_timestamps, V, max_initial)

extern "C" int f5e_whisper_beam_step_ts(hipStream_t st, const float* logits, long long ld_logits, const int* suppress, int n_sup,
                                        const int* begin_suppress, int n_beg, float* score, const int* hyp_in, const int* anc_in,
                                        int* hyp_out, int* anc_out, int ld, int* last, int* pool_hyp, int* pool_len,
                                        float* pool_score, int* pool_n, int* open, int* alive, void* scratch,
                                        unsigned long long scratch_bytes, int B, int K, int V, int p, int n0, int cap, int eos,
                                        float length_penalty, int no_timestamps, int max_initial, int* desc) {
  F5E_REQUIRE(desc, "whisper_beam_step_ts: null operand");
  F5E_TS_REQUIRE("whisper_beam_step_ts");
  return beam_step_impl(st, logits, ld_logits, suppress, n_sup, begin_suppress, n_beg, score, hyp_in, anc_in, hyp_out, anc_out, ld,
                        last, pool_hyp, pool_len, pool_score, pool_n, open, alive, scratch, scratch_bytes, B, K, V, p, n0, cap, eos,
                        length_penalty, desc, no_timestamps, max_initial);
}

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

static int ts_check(const char* name, const float* logits, long long ld, const int* suppress, int n_sup, const int* begin_suppress,
                    int n_beg, const int* tokens, int ld_tok, int R, int V, int p, int n0, int eos) {
  F5E_REQUIRE(logits && tokens, "%s: null operand", name);
  F5E_REQUIRE(R > 0 && R <= 0x7fffffff / 2 && V >= 2 && V <= GP_MAX_V && ld >= V,
              "%s: need R > 0, 2 <= V <= %d and ld >= V (R=%d V=%d)", name, GP_MAX_V, R, V);
  F5E_REQUIRE(n_sup >= 0 && n_beg >= 0 && (n_sup == 0 || suppress) && (n_beg == 0 || begin_suppress),
              "%s: a suppression list without its pointer", name);
  F5E_REQUIRE(n0 >= 1 && p >= n0 - 1 && ld_tok >= p + 2,
              "%s: need n0 >= 1, p >= n0 - 1 and token rows of at least p + 2 columns (n0=%d p=%d ld_tok=%d)", name, n0, p, ld_tok);
  F5E_REQUIRE(eos >= 0 && eos < V, "%s: need 0 <= eos < V", name);
  return F5E_OK;
}

extern "C" int f5e_whisper_ts_pick(hipStream_t st, const float* logits, long long ld, const int* suppress, int n_sup,
                                   const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int* last, int* done, int* alive,
                                   float* sum_logp, int R, int V, int p, int n0, int eos, int no_timestamps, int max_initial) {
  F5E_REQUIRE(last && done && alive && sum_logp, "whisper_ts_pick: null operand");
  const int rc = ts_check("whisper_ts_pick", logits, ld, suppress, n_sup, begin_suppress, n_beg, tokens, ld_tok, R, V, p, n0, eos);
  if (rc != F5E_OK) return rc;
  F5E_TS_REQUIRE("whisper_ts_pick");
  hipLaunchKernelGGL(ts_rule_kernel<true>, dim3((unsigned)R), dim3(256), 0, st, logits, ld, suppress, n_sup, begin_suppress,
                     p + 1 == n0 ? n_beg : 0, tokens, ld_tok, last, done, sum_logp, nullptr, V, p, n0, eos, no_timestamps,
                     max_initial);
  hipLaunchKernelGGL(alive_count_kernel, dim3(1), dim3(256), 0, st, done, alive, R);
  F5E_LAUNCH_CHECK("whisper_ts_pick");
  return F5E_OK;
}

extern "C" int f5e_whisper_sample_pick(hipStream_t st, const float* logits, long long ld, const int* suppress, int n_sup,
                                       const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int* last, int* done,
                                       int* alive, float* sum_logp, int R, int V, int p, int n0, int eos, int no_timestamps,
                                       int max_initial, float temperature, unsigned long long seed, const int* row_key,
                                       const int* serial) {
  F5E_REQUIRE(last && done && alive && sum_logp && row_key && serial, "whisper_sample_pick: null operand");
  const int rc = ts_check("whisper_sample_pick", logits, ld, suppress, n_sup, begin_suppress, n_beg, tokens, ld_tok, R, V, p, n0, eos);
  if (rc != F5E_OK) return rc;
  if (no_timestamps != -1) F5E_TS_REQUIRE("whisper_sample_pick");   // -1: without the timestamp rules
  F5E_REQUIRE(max_initial >= -1, "whisper_sample_pick: need max_initial >= -1 (got %d)", max_initial);
  F5E_REQUIRE(temperature > 0.f && temperature < __builtin_inff(), "whisper_sample_pick: need a finite temperature > 0 (got %g)",
              (double)temperature);
  hipLaunchKernelGGL(ts_sample_kernel, dim3((unsigned)R), dim3(256), 0, st, logits, ld, suppress, n_sup, begin_suppress,
                     p + 1 == n0 ? n_beg : 0, tokens, ld_tok, last, done, sum_logp, V, p, n0, eos, no_timestamps, max_initial,
                     temperature, (unsigned)seed, (unsigned)(seed >> 32), row_key, serial);
  hipLaunchKernelGGL(alive_count_kernel, dim3(1), dim3(256), 0, st, done, alive, R);
  F5E_LAUNCH_CHECK("whisper_sample_pick");
  return F5E_OK;
}

extern "C" int f5e_whisper_ts_rule(hipStream_t st, const float* logits, long long ld, const int* suppress, int n_sup,
                                   const int* begin_suppress, int n_beg, const int* tokens, int ld_tok, int* desc, int R, int V,
                                   int p, int n0, int eos, int no_timestamps, int max_initial) {
  F5E_REQUIRE(desc, "whisper_ts_rule: null operand");
  const int rc = ts_check("whisper_ts_rule", logits, ld, suppress, n_sup, begin_suppress, n_beg, tokens, ld_tok, R, V, p, n0, eos);
  if (rc != F5E_OK) return rc;
  F5E_TS_REQUIRE("whisper_ts_rule");
  hipLaunchKernelGGL(ts_rule_kernel<false>, dim3((unsigned)R), dim3(256), 0, st, logits, ld, suppress, n_sup, begin_suppress,
                     p + 1 == n0 ? n_beg : 0, const_cast<int*>(tokens), ld_tok, nullptr, nullptr, nullptr, desc, V, p, n0, eos,
                     no_timestamps, max_initial);
  F5E_LAUNCH_CHECK("whisper_ts_rule");
  return F5E_OK;
}
