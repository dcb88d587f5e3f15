// Paraformer (funasr paraformer-zh, the reference's Chinese WER recogniser; eval/paraformer.py): everything of the
// model that is not a GEMM, a LayerNorm, an im2col or a plain attention -- the LFR + CMVN front behind f5e_kaldi_fbank, the
// SANM attention's FSMN memory block, the CIF predictor's weights and scan, and the one-pass pick of the non-autoregressive
// decoder.  fp32, channels-last, per-row lengths DEVICE int [B] clamped to [0, T] (NULL: every row is full).  No allocation,
// no synchronisation, nothing read back, no atomics (every reduction runs in a fixed order): capturable, and a replay gives
// the bits of the eager run.  The unit is built with -ffp-contract=off: every product and every sum below is rounded on its own.
#include "f5e_common.h"
#include <math.h>

namespace {

constexpr int CIF_CHUNK = 4096;     // alpha values the scan holds in LDS at a time
constexpr int FSMN_MAX_K = 256;

__device__ __forceinline__ int row_len(const int* len, int b, int T) {
  const int n = len ? len[b] : T;
  return n < 0 ? 0 : (n > T ? T : n);
}

// ---- f5e_lfr_cmvn_f32: one output element per thread; no reductions.
__global__ __launch_bounds__(256) void pf_lfr_cmvn_kernel(const float* __restrict__ fbank, const int* __restrict__ count, int win,
                                                          int hop, const float* __restrict__ shift,
                                                          const float* __restrict__ scale, const float* __restrict__ pos,
                                                          float* __restrict__ out, int* __restrict__ frames_out, int T, int Tp,
                                                          int n_mels, int m, int n, float xscale, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int W = m * n_mels;
  const long long bt = e / W;
  const int k = (int)(e - bt * W), b = (int)(bt / Tp), i = (int)(bt - (long long)b * Tp);
  int Tb = count ? count[b] : T;
  if (count && hop > 0) Tb = Tb < win ? 0 : 1 + (Tb - win) / hop;     // count holds samples: kaldi's snip_edges frame count
  Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
  const int Tpb = (Tb + n - 1) / n;
  if (i == 0 && k == 0 && frames_out) frames_out[b] = Tpb;
  float v = 0.f;
  if (i < Tpb) {
    const int j = k / n_mels, c = k - j * n_mels;
    int f = n * i + j - (m - 1) / 2;             // frame of the sequence with (m - 1) / 2 copies of frame 0 in front
    f = f < 0 ? 0 : (f > Tb - 1 ? Tb - 1 : f);   // ... and the last frame repeated behind
    v = fbank[((long long)b * T + f) * n_mels + c];
    v = (v + shift[k]) * scale[k];
    v = v * xscale;
    if (pos) v = v + pos[(long long)i * W + k];
  }
  out[e] = v;
}

// ---- f5e_fsmn_f32: 4 channels per thread; the K taps in order, then the input itself, then the addend.
__global__ __launch_bounds__(256) void pf_fsmn_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w_t,
                                                      const int* __restrict__ len, const float* addend, int ld_add, float* out,
                                                      int ldo, int T, int C4, int K, int left, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long long bt = e / C4;
  const int c = (int)(e - bt * C4) * 4, b = (int)(bt / T), t = (int)(bt - (long long)b * T);
  const int n = row_len(len, b, T);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (t < n) {
    const float* xb = x + (long long)b * T * ldx + c;
    for (int j = 0; j < K; ++j) {
      const int s = t + j - left;
      if (s >= 0 && s < n) acc += *(const f32x4*)(w_t + (long long)j * C4 * 4 + c) * *(const f32x4*)(xb + (long long)s * ldx);
    }
    acc += *(const f32x4*)(xb + (long long)t * ldx);
  }
  if (addend) acc += *(const f32x4*)(addend + bt * ld_add + c);
  *(f32x4*)(out + bt * ldo + c) = acc;
}

// ---- f5e_mask_rows_f32
__global__ __launch_bounds__(256) void pf_mask_rows_kernel(float* __restrict__ x, int ldx, const int* __restrict__ len, int T,
                                                           int C, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long long bt = e / C;
  const int c = (int)(e - bt * C), b = (int)(bt / T), t = (int)(bt - (long long)b * T);
  if (t >= row_len(len, b, T)) x[bt * ldx + c] = 0.f;
}

// ---- f5e_cif_alpha_f32: one workgroup per row; the count is floor of the sum in double (fixed order: strided partials, then
// the 256 partials in ascending order)
__global__ __launch_bounds__(256) void pf_cif_alpha_kernel(const float* __restrict__ logit, int ldl, const int* __restrict__ len,
                                                           float* __restrict__ alpha, int lda, int* __restrict__ n_out, int T,
                                                           float smooth, float noise, float tail) {
  __shared__ double red[256];
  const int tid = threadIdx.x, b = blockIdx.x, n = row_len(len, b, T);
  double s = 0.0;
  for (int t = tid; t <= T; t += 256) {
    float a = 0.f;
    if (t < n) {
      const float sg = 1.0f / (1.0f + expf(-logit[((long long)b * T + t) * ldl]));
      a = fmaxf(sg * smooth - noise, 0.f);
    } else if (t == n) {
      a = tail;
    }
    alpha[(long long)b * lda + t] = a;
    s += (double)a;
  }
  red[tid] = s;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int i = 0; i < 256; ++i) tot += red[i];
    n_out[b] = (int)floor(tot);
  }
}

// ---- f5e_cif_fire_f32, phase 1: the scan of one row by ONE thread, its alpha staged through LDS by the workgroup.  Steps
// 0 .. len (the tail step included): len + 1 dependent additions, the sequential loop's own.
__global__ __launch_bounds__(256) void pf_cif_scan_kernel(const float* __restrict__ alpha, int lda, const int* __restrict__ len,
                                                          float* __restrict__ cur, int* __restrict__ pos, float* __restrict__ rem,
                                                          int* __restrict__ count, int T, int Lcap, float threshold) {
  __shared__ float sa[CIF_CHUNK], sc[CIF_CHUNK];
  const int tid = threadIdx.x, b = blockIdx.x, steps = row_len(len, b, T) + 1;
  float integrate = 0.f;
  int k = 0;
  for (int t0 = 0; t0 < steps; t0 += CIF_CHUNK) {
    const int m = steps - t0 < CIF_CHUNK ? steps - t0 : CIF_CHUNK;
    for (int i = tid; i < m; i += 256) sa[i] = alpha[(long long)b * lda + t0 + i];
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < m; ++i) {
        const float a = sa[i];
        const float comp = 1.0f - integrate;
        integrate = integrate + a;
        const bool fire = integrate >= threshold;
        if (fire) integrate = integrate - 1.0f;
        const float c = fire ? comp : a;
        sc[i] = c;
        if (fire) {
          if (k < Lcap) {
            pos[(long long)b * Lcap + k] = t0 + i;
            rem[(long long)b * Lcap + k] = a - c;
          }
          ++k;
        }
      }
    }
    __syncthreads();
    for (int i = tid; i < m; i += 256) cur[(long long)b * lda + t0 + i] = sc[i];
    __syncthreads();
  }
  if (tid == 0) count[b] = k;
}

// phase 2: token k of row b, one channel per thread: the predecessor's remainder, then the steps up to its own fire, in time
// order.  A step at or past len (the tail) has a zero hidden state by definition: h is not read there.
__global__ __launch_bounds__(256) void pf_cif_emit_kernel(const float* __restrict__ cur, int lda, const float* __restrict__ h,
                                                          int ldh, const int* __restrict__ len, const int* __restrict__ pos,
                                                          const float* __restrict__ rem, const int* __restrict__ count,
                                                          const int* __restrict__ n_limit, float* __restrict__ out, int ldo, int T,
                                                          int D, int Lcap) {
  const int k = blockIdx.x, b = blockIdx.y, n = row_len(len, b, T);
  int cnt = count[b] < Lcap ? count[b] : Lcap;
  if (n_limit) { const int lim = n_limit[b] < 0 ? 0 : n_limit[b]; cnt = cnt < lim ? cnt : lim; }
  const float* hb = h + (long long)b * T * ldh;
  const float* cb = cur + (long long)b * lda;
  int t0 = 0, t1 = -1, tp = -1;
  float rp = 0.f;
  if (k < cnt) {
    t1 = pos[(long long)b * Lcap + k];
    if (k > 0) { tp = pos[(long long)b * Lcap + k - 1]; rp = rem[(long long)b * Lcap + k - 1]; t0 = tp + 1; }
    t1 = t1 > n ? n : t1;     // the scan writes positions <= len; kept inside the row whatever the buffer holds
  }
  for (int c = threadIdx.x; c < D; c += blockDim.x) {
    float frame = 0.f;
    if (k < cnt) {
      if (tp >= 0) frame = __fmul_rn(rp, tp < n ? hb[(long long)tp * ldh + c] : 0.f);
      for (int t = t0; t <= t1; ++t)
        frame = __fadd_rn(frame, __fmul_rn(cb[t], t < n ? hb[(long long)t * ldh + c] : 0.f));
    }
    out[((long long)b * Lcap + k) * ldo + c] = frame;
  }
}

// ---- f5e_nar_pick, launch 1: one wave per token row, ONE pass over its logits: every lane carries a running maximum (first
// index on ties) and the sum of exp about it; the wave merges them.
__global__ __launch_bounds__(256) void pf_pick_rows_kernel(const float* __restrict__ logits, long long ld,
                                                           const int* __restrict__ n, int* __restrict__ arg,
                                                           float* __restrict__ lp, int R, int L, int V) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  const int b = r / L, k = r - b * L;
  if (n && k >= n[b]) {
    if (lane == 0) { arg[r] = -1; lp[r] = 0.f; }
    return;
  }
  const float* row = logits + (long long)r * ld;
  float m = -__builtin_inff(), s = 0.f;
  int a = WAVE_NONE;
  for (int v = lane; v < V; v += 64) {
    const float x = row[v];
    if (x > m) {
      s = s * expf(m - x) + 1.0f;
      m = x;
      a = v;
    } else {
      s += expf(x - m);
    }
  }
  float M = m;
  int A = a;
  wave_argmax(M, A);
  const float tot = wave_sum(a == WAVE_NONE ? 0.f : s * expf(m - M));
  if (lane == 0) { arg[r] = A == WAVE_NONE ? -1 : A; lp[r] = -logf(tot); }
}

// launch 2: one wave per utterance: the special ids dropped, the rest compacted in order, the score summed over all n tokens
__global__ __launch_bounds__(64) void pf_pick_compact_kernel(const int* __restrict__ arg, const float* __restrict__ lp,
                                                             const int* __restrict__ n, int* __restrict__ ids,
                                                             int* __restrict__ len_out, float* __restrict__ score, int L, int sos,
                                                             int eos, int blank, int pad) {
  const int lane = threadIdx.x, b = blockIdx.x;
  int nb = n ? n[b] : L;
  nb = nb < 0 ? 0 : (nb > L ? L : nb);
  int outn = 0;
  float sc = 0.f;
  for (int k0 = 0; k0 < nb; k0 += 64) {
    const int k = k0 + lane;
    const bool in = k < nb;
    const int id = in ? arg[(long long)b * L + k] : -1;
    if (in) sc += lp[(long long)b * L + k];
    const bool keep = in && id >= 0 && id != sos && id != eos && id != blank;
    const unsigned long long mask = __ballot(keep);
    if (keep) ids[(long long)b * L + outn + __popcll(mask & ((1ull << lane) - 1ull))] = id;
    outn += __popcll(mask);
  }
  for (int k = outn + lane; k < L; k += 64) ids[(long long)b * L + k] = pad;
  sc = wave_sum(sc);
  if (lane == 0) { len_out[b] = outn; score[b] = sc; }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned blocks256(long long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

extern "C" {

int f5e_lfr_cmvn_f32(hipStream_t st, const float* fbank, const int* count, int win, int hop, const float* shift,
                     const float* scale, const float* pos, int pos_rows, float* out, int* frames_out, int B, int T, int Tp,
                     int n_mels, int m, int n, float xscale) {
  F5E_REQUIRE(fbank && shift && scale && out, "lfr_cmvn_f32: null operand");
  F5E_REQUIRE(B > 0 && T > 0 && n_mels > 0 && m > 0 && n > 0 && m <= 64, "lfr_cmvn_f32: need B, T, n_mels, n > 0 and 0 < m <= 64");
  F5E_REQUIRE(Tp >= (T + n - 1) / n, "lfr_cmvn_f32: out holds %d rows per utterance, %d frames give %d", Tp, T, (T + n - 1) / n);
  F5E_REQUIRE(!pos || pos_rows >= Tp, "lfr_cmvn_f32: the position table has %d rows, fewer than %d", pos_rows, Tp);
  F5E_REQUIRE(hop >= 0 && (hop == 0 || win > 0), "lfr_cmvn_f32: hop must be >= 0 (0: count holds frames) and win > 0 with it");
  const long long total = (long long)B * Tp * m * n_mels;
  F5E_REQUIRE(total <= 0x7fffffffLL * 64, "lfr_cmvn_f32: B * T' * m * n_mels too large");
  hipLaunchKernelGGL(pf_lfr_cmvn_kernel, dim3(blocks256(total)), dim3(256), 0, st, fbank, count, win, hop, shift, scale, pos, out,
                     frames_out, T, Tp, n_mels, m, n, xscale, total);
  F5E_LAUNCH_CHECK("lfr_cmvn_f32");
  return F5E_OK;
}

int f5e_fsmn_f32(hipStream_t st, const float* x, int ldx, const float* w_t, const int* len, const float* addend, int ld_add,
                 float* out, int ldo, int B, int T, int C, int K, int left) {
  F5E_REQUIRE(x && w_t && out, "fsmn_f32: null operand");
  F5E_REQUIRE(B > 0 && T > 0 && C > 0 && C % 4 == 0, "fsmn_f32: need B, T > 0 and C a positive multiple of 4 (got %d)", C);
  F5E_REQUIRE(K >= 1 && K <= FSMN_MAX_K && left >= 0 && left <= K - 1, "fsmn_f32: need 1 <= K <= %d and 0 <= left <= K - 1",
              FSMN_MAX_K);
  F5E_REQUIRE(ldx >= C && ldo >= C && ldx % 4 == 0 && ldo % 4 == 0 && (!addend || (ld_add >= C && ld_add % 4 == 0)),
              "fsmn_f32: row strides must be multiples of 4 floats and at least C");
  F5E_REQUIRE(al16(x) && al16(w_t) && al16(out) && al16(addend), "fsmn_f32: operands must be 16-byte aligned");
  F5E_REQUIRE(x != (const float*)out, "fsmn_f32: in-place operation is not supported (neighbouring frames read x)");
  const long long total = (long long)B * T * (C / 4);
  F5E_REQUIRE(total <= 0x7fffffffLL * 64, "fsmn_f32: B * T * C too large");
  hipLaunchKernelGGL(pf_fsmn_kernel, dim3(blocks256(total)), dim3(256), 0, st, x, ldx, w_t, len, addend, ld_add, out, ldo, T, C / 4,
                     K, left, total);
  F5E_LAUNCH_CHECK("fsmn_f32");
  return F5E_OK;
}

int f5e_mask_rows_f32(hipStream_t st, float* x, int ldx, const int* len, int B, int T, int C) {
  F5E_REQUIRE(x && len, "mask_rows_f32: null operand");
  F5E_REQUIRE(B > 0 && T > 0 && C > 0 && ldx >= C, "mask_rows_f32: need B, T, C > 0 and ldx >= C");
  const long long total = (long long)B * T * C;
  F5E_REQUIRE(total <= 0x7fffffffLL * 64, "mask_rows_f32: B * T * C too large");
  hipLaunchKernelGGL(pf_mask_rows_kernel, dim3(blocks256(total)), dim3(256), 0, st, x, ldx, len, T, C, total);
  F5E_LAUNCH_CHECK("mask_rows_f32");
  return F5E_OK;
}

int f5e_cif_alpha_f32(hipStream_t st, const float* logits, int ld_logits, const int* len, float* alpha, int ld_alpha, int* n_out,
                      int B, int T, float smooth, float noise, float tail) {
  F5E_REQUIRE(logits && alpha && n_out, "cif_alpha_f32: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && ld_logits >= 1 && ld_alpha >= T + 1,
              "cif_alpha_f32: need 0 < B <= 65535, T > 0, ld_logits >= 1 and ld_alpha >= T + 1 (the tail step)");
  hipLaunchKernelGGL(pf_cif_alpha_kernel, dim3((unsigned)B), dim3(256), 0, st, logits, ld_logits, len, alpha, ld_alpha, n_out, T,
                     smooth, noise, tail);
  F5E_LAUNCH_CHECK("cif_alpha_f32");
  return F5E_OK;
}

int f5e_cif_fire_f32(hipStream_t st, const float* alpha, int ld_alpha, const float* h, int ldh, const int* len,
                     const int* n_limit, float* cur, int* pos, float* rem, int* count, float* out, int ldo, int B, int T, int D,
                     int L_cap, float threshold) {
  F5E_REQUIRE(alpha && h && cur && pos && rem && count && out, "cif_fire_f32: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && D > 0 && L_cap > 0 && L_cap <= 0x7fffffff / 2,
              "cif_fire_f32: need 0 < B <= 65535 and T, D, L_cap > 0");
  F5E_REQUIRE(ld_alpha >= T + 1 && ldh >= D && ldo >= D, "cif_fire_f32: need ld_alpha >= T + 1 (the tail step), ldh and ldo >= D");
  F5E_REQUIRE(cur != alpha, "cif_fire_f32: cur must not alias alpha");
  hipLaunchKernelGGL(pf_cif_scan_kernel, dim3((unsigned)B), dim3(256), 0, st, alpha, ld_alpha, len, cur, pos, rem, count, T, L_cap,
                     threshold);
  const int nt = D >= 256 ? 256 : (D + 63) / 64 * 64;
  hipLaunchKernelGGL(pf_cif_emit_kernel, dim3((unsigned)L_cap, (unsigned)B), dim3(nt), 0, st, cur, ld_alpha, h, ldh, len, pos, rem,
                     count, n_limit, out, ldo, T, D, L_cap);
  F5E_LAUNCH_CHECK("cif_fire_f32");
  return F5E_OK;
}

int f5e_nar_pick(hipStream_t st, const float* logits, long long ld, const int* n, int* arg, float* logp, int* ids, int* len_out,
                 float* score, int B, int L, int V, int sos, int eos, int blank, int pad) {
  F5E_REQUIRE(logits && arg && logp && ids && len_out && score, "nar_pick: null operand");
  F5E_REQUIRE(B > 0 && L > 0 && V > 0 && ld >= V && (long long)B * L <= 0x7fffffffLL / 4,
              "nar_pick: need B, L, V > 0, ld >= V and B * L below 2^29");
  const int R = B * L;
  hipLaunchKernelGGL(pf_pick_rows_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, logits, ld, n, arg, logp, R, L, V);
  hipLaunchKernelGGL(pf_pick_compact_kernel, dim3((unsigned)B), dim3(64), 0, st, arg, logp, n, ids, len_out, score, L, sos, eos,
                     blank, pad);
  F5E_LAUNCH_CHECK("nar_pick");
  return F5E_OK;
}

}  // extern "C"
