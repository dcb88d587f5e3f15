// Whisper's speculative decoding (assisted generation): the large model checks U drafted tokens in ONE pass per layer behind its
// existing cache, instead of U cached single-position steps.  fp32 throughout.
//
//   f5e_attn_append_f32    causal self-attention of the U new positions p0 .. p0+U-1 of R rows.  The wave tile of
//                          f5e_attn_prefill_f32 (one wave per (row, head, 16-query tile), S^T = K . Q^T and O^T = V^T . P^T on
//                          v_mfma_f32_16x16x4_f32).  The cached keys begin[r] .. p0-1 come from kc / vc in 16-key tiles from
//                          begin[r] & ~15, masked at both edges and not causally; the new keys 0 .. u come from qkv, never from
//                          the caches, under the causal mask; one online softmax runs across both.  The tile that owns 16 new
//                          positions of a head files their k and v in slots [r][p0 + u].  A launch reads slots below p0 only and
//                          writes slots p0 .. p0+U-1 only, so it reads nothing that it writes.
//   f5e_whisper_verify     the greedy (or ruled) pick of U + 1 positions per row at once: one workgroup per (row, position) runs
//                          the body of f5e_greedy_pick / f5e_whisper_ts_pick (whisper_pick.h) on that position's logits and on
//                          the history that ends there, drafts included.
//   f5e_whisper_accept     one launch: the longest agreed prefix per row, the common advance, the tokens, last, done, sum_logp,
//                          alive and the draft's table put right.
#include "f5e_common.h"
#include "whisper_pick.h"

namespace {

struct AppendArgs {
  const float* qkv;
  float *kc, *vc, *out;
  const int* begin;
  long long row_stride;
  int ld_qkv, pos_stride, ldo, U, HD, p0;
  float scale;
};

// One 16-key tile of the online softmax: kp / vp address the tile's keys and values (kp: this lane's key row, + 4 g; vp(i): the
// value row of key 4 g + i, + c16), vis[i]: key 4 g + i is visible to this lane's query.
template <int NB, class VRow>
__device__ __forceinline__ void append_tile(const float* kp, VRow vrow, const bool (&vis)[4], const f32x4 (&qa)[NB], f32x4 (&acc)[NB],
                                            float& m_run, float& l_run, float scale) {
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const f32x4 kf = *(const f32x4*)(kp + 16 * j);
#pragma unroll
    for (int i = 0; i < 4; ++i) s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[i], qa[j][i], s0, 0, 0, 0);
  }
  float p[4], mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = vis[i] ? s0[i] * scale : -INFINITY;
    mx = fmaxf(mx, p[i]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float m_new = fmaxf(m_run, mx);
  const float m_use = m_new == -INFINITY ? 0.f : m_new;     // a row with nothing visible yet: exp(-inf - 0) = 0
  const float alpha = __expf(m_run - m_use);
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = __expf(p[i] - m_use);
    sum += p[i];
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  l_run = l_run * alpha + sum;
  m_run = m_new;
#pragma unroll
  for (int j = 0; j < NB; ++j) acc[j] *= alpha;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float* vp = vrow(i);
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * j], p[i], acc[j], 0, 0, 0);
  }
}

template <int DK>
__global__ __launch_bounds__(64) void attn_append_kernel(AppendArgs a) {
  constexpr int NB = DK / 16;
  const int lane = threadIdx.x, c16 = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, hd = blockIdx.y, r = blockIdx.z;
  const int U = a.U, p0 = a.p0, hc = hd * DK;
  const size_t row0 = (size_t)r * U;
  const int lo = a.begin ? min(max(a.begin[r], 0), p0 + U) : 0;      // the first visible position of the row
  const int lo_u = max(lo - p0, 0);                                  // ... among the new ones
  const int q_last = min(q0 + 15, U - 1);
  const int qr = min(q0 + c16, U - 1);                    // this lane's query (clamped: loads stay in bounds)
  const bool q_in = q0 + c16 < U, q_ok = q_in && p0 + qr >= lo;
  const long long cache_row = (long long)r * a.row_stride;

  f32x4 qa[NB];
  {
    const float* qp = a.qkv + (row0 + qr) * a.ld_qkv + hc + 4 * g;
    float* kd = a.kc + cache_row + (long long)(p0 + qr) * a.pos_stride + hc + 4 * g;
    float* vd = a.vc + cache_row + (long long)(p0 + qr) * a.pos_stride + hc + 4 * g;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      qa[j] = *(const f32x4*)(qp + 16 * j);
      if (q_in) {                                         // the tile files its own positions, the padded ones included
        *(f32x4*)(kd + 16 * j) = *(const f32x4*)(qp + a.HD + 16 * j);
        *(f32x4*)(vd + 16 * j) = *(const f32x4*)(qp + 2 * a.HD + 16 * j);
      }
    }
  }
  f32x4 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  // the cached keys lo .. p0-1: no causal mask (every new query lies behind them); only slots below p0 are read
  if (p0 + q_last >= lo) {
    for (int kt = lo & ~15; kt < p0; kt += 16) {
      const int kr = min(kt + c16, p0 - 1);
      const float* kp = a.kc + cache_row + (long long)kr * a.pos_stride + hc + 4 * g;
      bool vis[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kt + 4 * g + i;
        vis[i] = q_ok && key >= lo && key < p0;
      }
      append_tile<NB>(kp, [&](int i) {
        const int vr = min(kt + 4 * g + i, p0 - 1);
        return (const float*)(a.vc + cache_row + (long long)vr * a.pos_stride + hc + c16);
      }, vis, qa, acc, m_run, l_run, a.scale);
    }
    // the new keys lo_u .. u, from qkv: the prefill's loop
    for (int kt = lo_u & ~15; kt <= q_last; kt += 16) {
      const int kr = min(kt + c16, U - 1);
      const float* kp = a.qkv + (row0 + kr) * a.ld_qkv + a.HD + hc + 4 * g;
      bool vis[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kt + 4 * g + i;
        vis[i] = q_ok && key >= lo_u && key <= qr;
      }
      append_tile<NB>(kp, [&](int i) {
        const int vr = min(kt + 4 * g + i, U - 1);
        return a.qkv + (row0 + vr) * a.ld_qkv + 2 * a.HD + hc + c16;
      }, vis, qa, acc, m_run, l_run, a.scale);
    }
  }
  if (q_in) {
    const float inv = (q_ok && l_run > 0.f) ? 1.0f / l_run : 0.f;   // a query below begin[r]: zeros
    float* op = a.out + (row0 + q0 + c16) * a.ldo + hc + 4 * g;
#pragma unroll
    for (int j = 0; j < NB; ++j) *(f32x4*)(op + 16 * j) = acc[j] * inv;
  }
}

// ---- verify: one workgroup per (position j, row r) -------------------------------------------------------------------------------
template <bool RULES>
__global__ __launch_bounds__(256) void verify_kernel(const float* __restrict__ logits, long long ld,
                                                     const int* __restrict__ suppress, int n_sup,
                                                     const int* __restrict__ begin_suppress, int n_beg,
                                                     const int* __restrict__ hist, int ld_hist, int* __restrict__ cand,
                                                     float* __restrict__ logp, int U1, int V, int p, int n0, int eos, int no_ts,
                                                     int max_initial) {
  __shared__ unsigned bits[GP_MAX_V / 32];
  __shared__ float rm[2][4], rs[2][4];
  __shared__ int ra[2][4], slot;
  const int tid = threadIdx.x, j = blockIdx.x, r = blockIdx.y;
  const int pj = p + j, words = (V + 31) / 32;
  const float* row = logits + ((size_t)r * U1 + j) * ld;
  const int nb = pj + 1 == n0 ? n_beg : 0;               // begin_suppress counts at the first generated position only
  for (int i = tid; i < words; i += 256) bits[i] = 0u;
  if (RULES) {
    const TsRule d = ts_rule_of(hist + (size_t)r * ld_hist + n0, pj + 1 - n0, V, no_ts + 1, max_initial, &slot);   // syncs twice
    pick_mark_bits(bits, suppress, n_sup, begin_suppress, nb, V);
    __syncthreads();
    const TsPick pk = ts_pick_row(row, bits, d, rm, rs, ra, V, eos, no_ts);
    if (tid == 0) cand[(size_t)r * U1 + j] = pk.arg, logp[(size_t)r * U1 + j] = pk.has ? pk.logp : 0.f;
  } else {
    __syncthreads();
    pick_mark_bits(bits, suppress, n_sup, begin_suppress, nb, V);
    __syncthreads();
    const int arg = greedy_pick_row(row, bits, rm[0], ra[0], V);
    if (tid == 0) cand[(size_t)r * U1 + j] = arg, logp[(size_t)r * U1 + j] = 0.f;
  }
}

// ---- accept: one workgroup, a thread per row ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void accept_kernel(const int* __restrict__ cand, const float* __restrict__ logp, int* hist,
                                                     int ld_hist, int* tokens, int ld_tok, int* last, int* done, int* alive,
                                                     float* sum_logp, int* adv, int R, int U, int p, int eos) {
  __shared__ int a_sh, any_sh, open_sh;
  const int tid = threadIdx.x, U1 = U + 1;
  if (tid == 0) a_sh = U1, any_sh = 0, open_sh = 0;
  __syncthreads();
  for (int r = tid; r < R; r += 256) {
    if (done[r]) continue;
    const int* c = cand + (size_t)r * U1;
    const int* h = hist + (size_t)r * ld_hist + p + 1;
    int m = 0;
    while (m < U && c[m] == h[m]) {
      ++m;
      if (c[m - 1] == eos) break;                        // nothing behind a closing eos is worth agreeing on
    }
    atomicMin(&a_sh, m + 1);
    any_sh = 1;
  }
  __syncthreads();
  const int a = any_sh ? a_sh : 1;                       // the common advance; no open row: one column of eos
  int n_open = 0;
  for (int r = tid; r < R; r += 256) {
    int* t = tokens + (size_t)r * ld_tok + p + 1;
    int* h = hist + (size_t)r * ld_hist + p + 1;
    const int* c = cand + (size_t)r * U1;
    const bool was_done = done[r] != 0;
    bool closed = was_done;
    float s = sum_logp ? sum_logp[r] : 0.f;
    for (int i = 0; i < a; ++i) {
      int tok = eos;
      if (!closed) {
        tok = c[i];
        s += logp[(size_t)r * U1 + i];                   // one addition per kept pick, in the order of the single steps
        if (tok == eos) closed = true;
      }
      t[i] = tok;
      h[i] = tok;
    }
    for (int i = a; i < U; ++i) h[i] = eos;              // the rejected drafts
    last[r] = t[a - 1];
    if (!was_done) {
      if (sum_logp) sum_logp[r] = s;
      if (closed) done[r] = 1;
    }
    n_open += closed ? 0 : 1;
  }
  if (n_open) atomicAdd(&open_sh, n_open);
  __syncthreads();
  if (tid == 0) *alive = open_sh, adv[0] = a;
}

}  // namespace

int f5e_attn_append_f32(hipStream_t st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride, int pos_stride,
                        const int* begin, float* out, int ldo, int R, int U, int Umax, int H, int dk, int p0, float scale) {
  F5E_REQUIRE(qkv && kc && vc && out, "attn_append_f32: null operand");
  F5E_REQUIRE(R > 0 && R <= 65535 && H > 0 && H <= 65535, "attn_append_f32: need 0 < R, H <= 65535");
  F5E_REQUIRE(dk == 16 || dk == 32 || dk == 64 || dk == 128, "attn_append_f32: head dim %d is not built (16, 32, 64 and 128 are)",
              dk);
  F5E_REQUIRE(Umax > 0 && Umax <= 4096 && U >= 1 && p0 >= 0 && (long long)p0 + U <= Umax,
              "attn_append_f32: need U >= 1, p0 >= 0 and p0 + U <= Umax <= 4096 (p0=%d U=%d Umax=%d)", p0, U, Umax);
  const long long HD = (long long)H * dk;
  F5E_REQUIRE(ld_qkv >= 3 * HD && ldo >= HD && pos_stride >= HD && row_stride >= (long long)(Umax - 1) * pos_stride + HD,
              "attn_append_f32: a stride is smaller than the data it spans");
  F5E_REQUIRE(ld_qkv % 4 == 0 && ldo % 4 == 0 && pos_stride % 4 == 0 && row_stride % 4 == 0 &&
                  (((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)out) & 15) == 0,
              "attn_append_f32: strides must be multiples of 4 floats, qkv, kc, vc and out 16-byte aligned");
  const AppendArgs a{qkv, kc, vc, out, begin, row_stride, ld_qkv, pos_stride, ldo, U, (int)HD, p0, scale};
  const dim3 grid((unsigned)((U + 15) / 16), (unsigned)H, (unsigned)R);
  switch (dk) {
    case 16: hipLaunchKernelGGL(attn_append_kernel<16>, grid, dim3(64), 0, st, a); break;
    case 32: hipLaunchKernelGGL(attn_append_kernel<32>, grid, dim3(64), 0, st, a); break;
    case 64: hipLaunchKernelGGL(attn_append_kernel<64>, grid, dim3(64), 0, st, a); break;
    default: hipLaunchKernelGGL(attn_append_kernel<128>, grid, dim3(64), 0, st, a); break;
  }
  F5E_LAUNCH_CHECK("attn_append_f32");
  return F5E_OK;
}

int f5e_whisper_verify(hipStream_t st, const float* logits, long long ld, const int* suppress, int n_sup, const int* begin_suppress,
                       int n_beg, const int* hist, int ld_hist, int* cand, float* logp, int R, int U, int V, int p, int n0, int eos,
                       int no_timestamps, int max_initial) {
  F5E_REQUIRE(logits && hist && cand && logp, "whisper_verify: null operand");
  F5E_REQUIRE(R > 0 && R <= 65535 && U >= 0 && U < 65535 && V >= 2 && V <= GP_MAX_V && ld >= V,
              "whisper_verify: need 0 < R <= 65535, 0 <= U < 65535, 2 <= V <= %d and ld >= V (R=%d U=%d V=%d)", GP_MAX_V, R, U, V);
  F5E_REQUIRE(n_sup >= 0 && n_beg >= 0 && (n_sup == 0 || suppress) && (n_beg == 0 || begin_suppress),
              "whisper_verify: a suppression list without its pointer");
  F5E_REQUIRE(n0 >= 1 && p >= n0 - 1 && (long long)p + U + 1 <= ld_hist,
              "whisper_verify: need n0 >= 1, p >= n0 - 1 and history rows of at least p + U + 1 columns (n0=%d p=%d U=%d ld=%d)", n0, p,
              U, ld_hist);
  F5E_REQUIRE(eos >= 0 && eos < V, "whisper_verify: need 0 <= eos < V");
  F5E_REQUIRE(max_initial >= -1, "whisper_verify: need max_initial >= -1 (got %d)", max_initial);
  const dim3 grid((unsigned)(U + 1), (unsigned)R);
  if (no_timestamps == -1) {                              // plain greedy rules
    hipLaunchKernelGGL(verify_kernel<false>, grid, dim3(256), 0, st, logits, ld, suppress, n_sup, begin_suppress, n_beg, hist,
                       ld_hist, cand, logp, U + 1, V, p, n0, eos, -1, -1);
  } else {
    F5E_REQUIRE(no_timestamps >= 0 && no_timestamps + 1 < V && eos <= no_timestamps,
                "whisper_verify: need 0 <= eos <= no_timestamps < V - 1 (eos=%d no_timestamps=%d V=%d)", eos, no_timestamps, V);
    hipLaunchKernelGGL(verify_kernel<true>, grid, dim3(256), 0, st, logits, ld, suppress, n_sup, begin_suppress, n_beg, hist,
                       ld_hist, cand, logp, U + 1, V, p, n0, eos, no_timestamps, max_initial);
  }
  F5E_LAUNCH_CHECK("whisper_verify");
  return F5E_OK;
}

int f5e_whisper_accept(hipStream_t st, const int* cand, const float* logp, int* hist, int ld_hist, int* tokens, int ld_tok,
                       int* last, int* done, int* alive, float* sum_logp, int* adv, int R, int U, int p, int eos) {
  F5E_REQUIRE(cand && logp && hist && tokens && last && done && alive && adv, "whisper_accept: null operand");
  F5E_REQUIRE(R > 0 && U >= 1 && p >= 0 && (long long)p + U + 2 <= ld_tok && (long long)p + U + 2 <= ld_hist,
              "whisper_accept: need R > 0, U >= 1, p >= 0, token and history rows of at least p + U + 2 "
              "columns (R=%d U=%d p=%d ld_tok=%d ld_hist=%d)", R, U, p, ld_tok, ld_hist);
  hipLaunchKernelGGL(accept_kernel, dim3(1), dim3(256), 0, st, cand, logp, hist, ld_hist, tokens, ld_tok, last, done, alive,
                     sum_logp, adv, R, U, p, eos);
  F5E_LAUNCH_CHECK("whisper_accept");
  return F5E_OK;
}
