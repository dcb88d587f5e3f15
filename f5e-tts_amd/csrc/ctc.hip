// CTC decoding on the device: forced alignment (f5e_ctc_align), best-path search (f5e_ctc_greedy) and the likelihood of a
// transcript (f5e_ctc_loss) over the scores of the ASR model's CTC head.  Replaces the reference's host routes:
// wenet/utils/ctc_util.py::forced_align (a Python double loop that builds a tensor per cell) and
// ASRModel.ctc_greedy_search (asr_model.py:416-459: log_softmax, topk, D2H, a Python collapse per utterance).
//
// ---- f5e_ctc_align.  The extended sequence ext has S = 2 l + 1 states (blank, y0, blank, y1, ..., blank).
//   alpha[0][0] = scores[0][blank], alpha[0][1] = scores[0][y0], everything else -inf;
//   alpha[t][s] = max(alpha[t-1][s], alpha[t-1][s-1] (s >= 1), alpha[t-1][s-2] (skip allowed)) + scores[t][ext[s]],
// one fp32 max and one fp32 add, the first maximum winning (torch.argmax), "skip allowed" = ext[s] is a label, s >= 2 and
// ext[s] != ext[s-2].  State 0 can only stay: the reference's log_alpha[t-1, s-1] at s = 0 is a negative index, i.e. the
// LAST state, which lets a path leave the final blank and run through the labels again; that is not CTC and not built.
//
// The mapping is the one of mas.hip (the same class of recurrence: serial in t, parallel in s):
//   * one workgroup per sequence; states are dealt to waves in runs of 64 (slot c of wave w = states (w * CPT + c) * 64 +
//     lane), the previous row lives in registers;
//   * s-1 comes from a one-lane wave rotate (DPP wave_ror:1), lane 0 taking lane 63 of the slot before it; s-2 is the same
//     shift applied to the shifted row.  Up to 256 states ONE wave carries the row: no LDS, no barrier.  Wider rows use up
//     to 16 waves of 4 slots; only the last TWO states of a wave cross waves, through a double-buffered LDS pair and one
//     barrier per row (row t reads buffer (t - 1) & 1 and writes t & 1);
//   * ext[s], "skip allowed" and "state exists" are loop-invariant registers; the emission gathers scores[t][ext[s]] are
//     fetched CTC_R rows ahead into registers (plain loads, they survive the barrier);
//   * the forward pass leaves TWO decision bits per state (how many states back the best predecessor lies) as two ballot
//     words per slot; the backtrack never reads an alpha.  Wave 0 resolves 64 rows per round: lane l fetches, for row
//     t0 - l, the three word pairs that cover states top - 127 .. top (the state moves by at most two per row), funnel-shifts
//     them into a 128-state window and parks it in LDS; a 64-step walk then reads one LDS word pair per step (a broadcast
//     read, no global load on the dependent chain).  T / 64 dependent load rounds instead of T.
// scores is only read.  Nothing is allocated or synchronised; the lengths are read on the device.
//
// ---- f5e_ctc_greedy.  Kernel 1: one wave per frame, argmax over V (the lowest index among equal maxima) and
// max - logsumexp, the raw ids parked in `hyp`.  Kernel 2: one workgroup per sequence collapses its row in place (keep frame
// t iff its id is not blank and differs from frame t-1's), compacting with ballot / popcount prefix sums, 1024 frames per
// round in frame order (a kept id lands at or before its own frame, and a round reads its frames before it writes).
//
// ---- f5e_ctc_loss.  log P(labels | frames) = log of the sum over ALL CTC paths: wenet/transformer/ctc.py::CTC.forward
// (torch.nn.CTCLoss, reduction "sum") per utterance and negated.  The recurrence of f5e_ctc_align with logaddexp in place
// of max, on log-probabilities lp[t][v] = scores[t][v] - logsumexp(scores[t][:]):
//   alpha[0][0] = lp[0][blank], alpha[0][1] = lp[0][y0], everything else -inf;
//   alpha[t][s] = logaddexp(alpha[t-1][s], alpha[t-1][s-1], alpha[t-1][s-2] (skip allowed)) + lp[t][ext[s]],
//   logp = logaddexp(alpha[t_len-1][S-1], alpha[t_len-1][S-2]),
// fp32, logaddexp(a, b) = max + log1p(exp(-|a - b|)) applied pairwise ((stay, s-1), then s-2); two -inf give -inf.  "Skip
// allowed" = ext[s] is a label, s >= 3 and the label differs from the one before it: adjacent equal labels are ordinary
// input here (they need a blank between them), and l = 0 (S = 1, the all-blank path) is legal.
// Kernel 1: one wave per frame < t_len writes logsumexp of the row into the workspace (max + log1p(sum over the OTHER
// classes of exp(x - max)), as f5e_ctc_greedy's frame_logp; 0 for a row of -inf, which keeps its lp at -inf).  It is a launch
// of its own because inside the serial kernel a V-wide reduction would sit on the dependent chain of every frame.
// Kernel 2: the mapping of ctc_align_kernel (states dealt to lanes in runs of 64, wave_ror1 for s-1 and s-2, one wave up to
// 256 states, beyond that up to 16 waves and the LDS pair with one barrier per row, emissions and the row's normaliser
// fetched CTC_R rows ahead) without the decision words and the backtrack.
#include "f5e_common.h"

namespace {

constexpr int CTC_R = 8;            // rows of emissions in flight per thread (x CPT registers, twice)
constexpr int CTC_MAX_L = 2047;     // S = 2 L + 1 <= 4095 states <= 16 waves x 4 slots x 64
constexpr int CTC_MAX_T = 16384;


template <int CPT, bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_align_kernel(
    const float* __restrict__ scores, long long batch_stride, int ld, const int* __restrict__ labels, int ld_lab,
    const int* __restrict__ t_len_p, const int* __restrict__ l_len_p, int blank, int* __restrict__ align_out,
    int* __restrict__ tok_start, int* __restrict__ tok_end, float* __restrict__ score_out,
    unsigned long long* __restrict__ dec, int T, int L, int V, int W64) {
  __shared__ float edge[2][16][2];                   // alpha of the last / second-to-last state of every wave
  __shared__ float fin[2];                           // alpha[t_len - 1][S - 1], [S - 2]
  __shared__ int n_bad;                              // adjacent equal labels + labels outside [0, V)
  __shared__ unsigned long long win[64][4];          // backtrack: per row, 128 states x 2 decision bits
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nt = blockDim.x;
  const int t_len = t_len_p[b], l_len = l_len_p[b];
  const int* lab = labels + (long long)b * ld_lab;
  int* al = align_out + (long long)b * T;

  if (tid == 0) n_bad = 0;
  __syncthreads();
  const bool in_range = l_len >= 1 && l_len <= L && t_len >= 1 && t_len <= T;
  int repeats = 0;
  if (in_range) {
    int bad = 0;
    for (int i = tid; i < l_len; i += nt) {
      const int y = lab[i];
      if (y < 0 || y >= V) bad += 1 << 16;           // a label that is no class: no path (and no gather out of the row)
      else if (i > 0 && y == lab[i - 1]) bad += 1;
    }
    if (bad) atomicAdd(&n_bad, bad);
    __syncthreads();
    repeats = n_bad;
  }
  // no CTC path (or lengths beyond the buffers): -1 / 0 / -inf rows, defined and harmless
  const bool valid = in_range && repeats < (1 << 16) && t_len >= l_len + repeats;   // workgroup-uniform
  for (int t = (valid ? t_len : 0) + tid; t < T; t += nt) al[t] = -1;
  // spans: all zero first (also those of labels < l_len: with true -inf in the scores every alpha can end at -inf, and
  // the backtrack then never visits some label); the backtrack's writes come after the barrier that ends the forward pass
  if (tok_start)
    for (int i = tid; i < L; i += nt) tok_start[(long long)b * L + i] = 0;
  if (tok_end)
    for (int i = tid; i < L; i += nt) tok_end[(long long)b * L + i] = 0;
  if (!valid) {
    if (score_out && tid == 0) score_out[b] = -__builtin_inff();
    return;
  }

  const float NEG = -__builtin_inff();
  const float* E = scores + (long long)b * batch_stride;
  unsigned long long* D = dec + (long long)b * T * W64 * 2;
  const int S = 2 * l_len + 1;
  int cls[CPT];
  bool live[CPT], skip[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int s = (w * CPT + c) * 64 + lane;
    live[c] = s < S;
    const bool is_lab = live[c] && (s & 1);
    const int y = is_lab ? lab[s >> 1] : blank;
    cls[c] = y;
    skip[c] = is_lab && s >= 3 && y != blank && y != lab[(s >> 1) - 1];
  }

  float prev[CPT], cur[CTC_R][CPT], nxt[CTC_R][CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) prev[c] = NEG;

  auto load_rows = [&](float (&dst)[CTC_R][CPT], int t0) {
#pragma unroll
    for (int r = 0; r < CTC_R; ++r) {
      const float* row = E + (long long)min(t0 + r, t_len - 1) * ld;
#pragma unroll
      for (int c = 0; c < CPT; ++c) dst[r][c] = row[cls[c]];
    }
  };

  // x shifted by one state: out[s] = x[s - 1]; e = x of the last state of the wave to the left
  auto shift = [&](const float (&x)[CPT], float e, float (&out)[CPT]) {
    float rot[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) rot[c] = wave_ror1(x[c]);
#pragma unroll
    for (int c = 0; c < CPT; ++c) out[c] = lane > 0 ? rot[c] : (c > 0 ? rot[c > 0 ? c - 1 : 0] : e);
  };

  auto step = [&](int t, const float (&em)[CPT]) {
    if (t == 0) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) prev[c] = (w * CPT + c) * 64 + lane < 2 ? em[c] : NEG;   // S >= 3: both states exist
    } else {
      float e1 = NEG, e2 = NEG;
      if (MULTI && w > 0) {
        e1 = edge[(t + 1) & 1][w - 1][0];
        e2 = edge[(t + 1) & 1][w - 1][1];
      }
      float p1[CPT], p2[CPT];
      shift(prev, e1, p1);       // alpha[t-1][s-1]; state 0 gets e1 = -inf (it can only stay)
      shift(p1, e2, p2);         // alpha[t-1][s-2]
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        float best = prev[c];
        int d = 0;
        if (p1[c] > best) best = p1[c], d = 1;
        if (skip[c] && p2[c] > best) best = p2[c], d = 2;
        const unsigned long long b0 = __ballot(d == 1), b1 = __ballot(d == 2);
        // a row of the scratch holds W64 = ceil((2 L + 1) / 64) word pairs, fewer than threads * CPT slots when L is small
        const int wi = w * CPT + c;
        if (lane == 0 && wi < W64) {
          D[((long long)t * W64 + wi) * 2] = b0;
          D[((long long)t * W64 + wi) * 2 + 1] = b1;
        }
        prev[c] = live[c] ? best + em[c] : NEG;
      }
    }
    if (MULTI) {
      if (lane == 63) edge[t & 1][w][0] = prev[CPT - 1];
      if (lane == 62) edge[t & 1][w][1] = prev[CPT - 1];
      __syncthreads();
    }
  };

  auto steps = [&](int t0, const float (&rows)[CTC_R][CPT]) {
#pragma unroll
    for (int r = 0; r < CTC_R; ++r)
      if (t0 + r < t_len) step(t0 + r, rows[r]);   // workgroup-uniform
  };
  load_rows(cur, 0);
  for (int t0 = 0; t0 < t_len; t0 += 2 * CTC_R) {   // the two register sets swap roles: no copies
    load_rows(nxt, t0 + CTC_R);
    steps(t0, cur);
    load_rows(cur, t0 + 2 * CTC_R);
    steps(t0 + CTC_R, nxt);
  }

#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int s = (w * CPT + c) * 64 + lane;
    if (s == S - 1) fin[0] = prev[c];
    if (s == S - 2) fin[1] = prev[c];
  }
  // The decision words are read back by wave 0 of this workgroup: a workgroup-scope release, then the barrier.
  __threadfence_block();
  __syncthreads();
  if (w != 0) return;

  const bool last_blank = fin[0] >= fin[1];
  if (score_out && lane == 0) score_out[b] = last_blank ? fin[0] : fin[1];
  int top = last_blank ? S - 1 : S - 2;   // state of frame t0 (wave-uniform)
  int above = -1;                          // state of frame t0 + 1 (none above the last frame)
  for (int t0 = t_len - 1; t0 >= 0; t0 -= 64) {
    const int t = t0 - lane;
    const int cbase = top - 127;           // state of window bit 0; may be negative (those bits are never set or used)
    const int wa = cbase >> 6, sh = cbase & 63;
    unsigned long long q[3][2] = {{0, 0}, {0, 0}, {0, 0}};
    if (t >= 1) {                          // row 0 holds no decision: its window stays 0
      const unsigned long long* drow = D + (long long)t * W64 * 2;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int wi = wa + k;
        if (wi >= 0 && wi < W64 && (k < 2 || sh != 0)) {
          q[k][0] = drow[wi * 2];
          q[k][1] = drow[wi * 2 + 1];
        }
      }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      win[lane][p] = sh ? (q[0][p] >> sh) | (q[1][p] << (64 - sh)) : q[0][p];          // states cbase .. cbase + 63
      win[lane][2 + p] = sh ? (q[1][p] >> sh) | (q[2][p] << (64 - sh)) : q[1][p];      // states cbase + 64 .. cbase + 127
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    int p = 127, mine = 0;
    for (int l = 0; l < 64; ++l) {
      const int half = p >> 6, bit = p & 63;
      const unsigned long long lo = win[l][half * 2], hi = win[l][half * 2 + 1];
      if (lane == l) mine = cbase + p;
      p -= (int)((lo >> bit) & 1ull) + 2 * (int)((hi >> bit) & 1ull);
    }
    __builtin_amdgcn_wave_barrier();       // the next round's windows overwrite what this walk read
    const int next_top = cbase + p;        // state of frame t0 - 64
    int up = __shfl_up(mine, 1, 64);       // state of frame t + 1
    if (lane == 0) up = above;
    int down = __shfl_down(mine, 1, 64);   // state of frame t - 1
    if (lane == 63) down = next_top;
    if (t >= 0) {
      const int s = min(max(mine, 0), S - 1);
      al[t] = (s & 1) ? lab[s >> 1] : blank;
      if (s & 1) {   // a token's own run is contiguous on a CTC path: one frame opens it, one closes it
        if (tok_start && (t == 0 || down != mine)) tok_start[(long long)b * L + (s >> 1)] = t;
        if (tok_end && up != mine) tok_end[(long long)b * L + (s >> 1)] = t + 1;
      }
    }
    above = __builtin_amdgcn_readlane(mine, 63);
    top = next_top;
  }
}

template <int CPT, bool MULTI>
void ctc_align_launch(hipStream_t st, int threads, const float* scores, long long batch_stride, int ld, const int* labels,
                      int ld_lab, const int* t_len, const int* l_len, int blank, int* align, int* tok_start, int* tok_end,
                      float* score, unsigned long long* dec, int B, int T, int L, int V, int W64) {
  hipLaunchKernelGGL((ctc_align_kernel<CPT, MULTI>), dim3((unsigned)B), dim3((unsigned)threads), 0, st, scores, batch_stride,
                     ld, labels, ld_lab, t_len, l_len, blank, align, tok_start, tok_end, score, dec, T, L, V, W64);
}

// ---------------------------------------------------------------- greedy

// one wave per frame: argmax over V (lowest index among equal maxima) and max - logsumexp
__global__ __launch_bounds__(256) void ctc_frame_argmax_kernel(const float* __restrict__ scores, long long batch_stride, int ld,
                                                                int* __restrict__ ids, float* __restrict__ frame_logp, int T,
                                                                int V) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (t >= T) return;   // wave-uniform
  const float* row = scores + (long long)b * batch_stride + (long long)t * ld;
  float m = -__builtin_inff();
  int arg = WAVE_NONE;
  for (int v = lane; v < V; v += 64) {
    const float x = row[v];
    if (x > m) m = x, arg = v;   // ascending v per lane: the first maximum stays
  }
  wave_argmax(m, arg);
  if (arg == WAVE_NONE) arg = 0;   // a row of -inf / NaN: class 0, like an argmax over equal values
  if (frame_logp) {                 // wave-uniform
    // max - logsumexp = -log(1 + sum over the OTHER classes of exp(x - max)): the winner's own term is exactly 1, and a
    // confident frame's log-probability is close to 0, where log(sum) would keep only the bits of 1 + eps that fp32 holds
    float sum = 0.f;
    for (int v = lane; v < V; v += 64) sum += v == arg ? 0.f : expf(row[v] - m);
    sum = wave_sum(sum);
    if (lane == 0) frame_logp[(long long)b * T + t] = -log1pf(sum);
  }
  if (lane == 0) ids[(long long)b * T + t] = arg;
}

// one workgroup per sequence: collapse the raw ids of `hyp` in place
__global__ __launch_bounds__(1024) void ctc_collapse_kernel(int* __restrict__ hyp, int* __restrict__ hyp_len,
                                                             const int* __restrict__ t_len_p, int blank, int pad_id, int T) {
  __shared__ int wave_cnt[16];
  __shared__ int carry_last;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int* row = hyp + (long long)b * T;
  const int t_len = min(max(t_len_p[b], 0), T);
  const int n = pad_id >= 0 ? T : t_len;   // frames that take part
  int count = 0;                           // workgroup-uniform
  if (tid == 0) carry_last = -1;           // no frame before the first: -1 is no class
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int t = base + tid;
    int id = -1, before = -1;
    if (t < n) {
      id = t < t_len ? row[t] : pad_id;
      before = t > base ? (t - 1 < t_len ? row[t - 1] : pad_id) : carry_last;
    }
    const bool keep = t < n && id != blank && id != before;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[w] = __popcll(m);
    __syncthreads();                       // every id of this round is in registers; carry_last has been read
    int off = count, total = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int c = wave_cnt[k];
      off += k < w ? c : 0;
      total += c;
    }
    if (keep) row[off + __popcll(m & ((1ull << lane) - 1ull))] = id;   // off + rank <= t
    if (t == min(base + 1023, n - 1)) carry_last = id;
    count += total;
    __syncthreads();
  }
  for (int t = count + tid; t < T; t += 1024) row[t] = -1;
  if (tid == 0) hyp_len[b] = count;
}

// ---------------------------------------------------------------- loss (sum over paths)

// one wave per frame < t_len: logsumexp over V into lse[b][t]
__global__ __launch_bounds__(256) void ctc_frame_lse_kernel(const float* __restrict__ scores, long long batch_stride, int ld,
                                                             const int* __restrict__ t_len_p, float* __restrict__ lse, int T,
                                                             int V) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (t >= T || t >= t_len_p[b]) return;   // wave-uniform
  const float* row = scores + (long long)b * batch_stride + (long long)t * ld;
  float m = -__builtin_inff();
  int arg = 0x7fffffff;
  for (int v = lane; v < V; v += 64) {
    const float x = row[v];
    if (x > m) m = x, arg = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {   // wave_argmax written out: with the call this launch measured 0.2 % slower per f5e_ctc_loss
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(arg, o, 64);
    if (om > m || (om == m && oa < arg)) m = om, arg = oa;
  }
  // the winner's own term is exactly 1: log1p of the rest keeps the bits that log(1 + eps) would drop on a confident frame
  float sum = 0.f;
  if (arg != 0x7fffffff)                   // wave-uniform; a row of -inf has no winner (x - m would be NaN)
    for (int v = lane; v < V; v += 64) sum += v == arg ? 0.f : expf(row[v] - m);
  sum = wave_sum(sum);
  if (lane == 0) lse[(long long)b * T + t] = arg != 0x7fffffff ? m + log1pf(sum) : 0.f;
}

template <int CPT, bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_loss_kernel(
    const float* __restrict__ scores, long long batch_stride, int ld, const int* __restrict__ labels, int ld_lab,
    const int* __restrict__ t_len_p, const int* __restrict__ l_len_p, int blank, float* __restrict__ logp,
    const float* __restrict__ lse, int T, int L, int V) {
  __shared__ float edge[2][16][2];                   // alpha of the last / second-to-last state of every wave
  __shared__ float fin[2];                           // alpha[t_len - 1][S - 1], [S - 2]
  __shared__ int n_bad;                              // adjacent equal labels + labels outside [0, V)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nt = blockDim.x;
  const int t_len = t_len_p[b], l_len = l_len_p[b];
  const int* lab = labels + (long long)b * ld_lab;
  const float NEG = -__builtin_inff();

  if (tid == 0) n_bad = 0, fin[0] = NEG, fin[1] = NEG;   // S = 1 has no state S - 2
  __syncthreads();
  const bool in_range = l_len >= 0 && l_len <= L && t_len >= 1 && t_len <= T;
  int repeats = 0;
  if (in_range) {
    int bad = 0;
    for (int i = tid; i < l_len; i += nt) {
      const int y = lab[i];
      if (y < 0 || y >= V) bad += 1 << 16;           // a label that is no class: no path (and no gather out of the row)
      else if (i > 0 && y == lab[i - 1]) bad += 1;   // equal neighbours need a blank frame between them
    }
    if (bad) atomicAdd(&n_bad, bad);
    __syncthreads();
    repeats = n_bad;
  }
  if (!(in_range && repeats < (1 << 16) && t_len >= l_len + repeats)) {   // workgroup-uniform: no CTC path
    if (tid == 0) logp[b] = NEG;
    return;
  }

  const float* E = scores + (long long)b * batch_stride;
  const float* N = lse + (long long)b * T;
  const int S = 2 * l_len + 1;
  int cls[CPT];
  bool live[CPT], skip[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int s = (w * CPT + c) * 64 + lane;
    live[c] = s < S;
    const bool is_lab = live[c] && (s & 1);
    const int y = is_lab ? lab[s >> 1] : blank;
    cls[c] = y;
    skip[c] = is_lab && s >= 3 && y != lab[(s >> 1) - 1];
  }

  float prev[CPT], cur[CTC_R][CPT], nxt[CTC_R][CPT], cur_n[CTC_R], nxt_n[CTC_R];
#pragma unroll
  for (int c = 0; c < CPT; ++c) prev[c] = NEG;

  auto load_rows = [&](float (&dst)[CTC_R][CPT], float (&norm)[CTC_R], int t0) {
#pragma unroll
    for (int r = 0; r < CTC_R; ++r) {
      const int t = min(t0 + r, t_len - 1);
      const float* row = E + (long long)t * ld;
      norm[r] = N[t];
#pragma unroll
      for (int c = 0; c < CPT; ++c) dst[r][c] = row[cls[c]];
    }
  };

  // x shifted by one state: out[s] = x[s - 1]; e = x of the last state of the wave to the left
  auto shift = [&](const float (&x)[CPT], float e, float (&out)[CPT]) {
    float rot[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) rot[c] = wave_ror1(x[c]);
#pragma unroll
    for (int c = 0; c < CPT; ++c) out[c] = lane > 0 ? rot[c] : (c > 0 ? rot[c > 0 ? c - 1 : 0] : e);
  };

  auto step = [&](int t, const float (&em)[CPT], float norm) {
    if (t == 0) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) prev[c] = (w * CPT + c) * 64 + lane < 2 && live[c] ? em[c] - norm : NEG;
    } else {
      float e1 = NEG, e2 = NEG;
      if (MULTI && w > 0) {
        e1 = edge[(t + 1) & 1][w - 1][0];
        e2 = edge[(t + 1) & 1][w - 1][1];
      }
      float p1[CPT], p2[CPT];
      shift(prev, e1, p1);       // alpha[t-1][s-1]; state 0 gets e1 = -inf (it can only stay)
      shift(p1, e2, p2);         // alpha[t-1][s-2]
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const float sum = logaddexp_f(logaddexp_f(prev[c], p1[c]), skip[c] ? p2[c] : NEG);
        prev[c] = live[c] ? sum + (em[c] - norm) : NEG;
      }
    }
    if (MULTI) {
      if (lane == 63) edge[t & 1][w][0] = prev[CPT - 1];
      if (lane == 62) edge[t & 1][w][1] = prev[CPT - 1];
      __syncthreads();
    }
  };

  auto steps = [&](int t0, const float (&rows)[CTC_R][CPT], const float (&norm)[CTC_R]) {
#pragma unroll
    for (int r = 0; r < CTC_R; ++r)
      if (t0 + r < t_len) step(t0 + r, rows[r], norm[r]);   // workgroup-uniform
  };
  load_rows(cur, cur_n, 0);
  for (int t0 = 0; t0 < t_len; t0 += 2 * CTC_R) {   // the two register sets swap roles: no copies
    load_rows(nxt, nxt_n, t0 + CTC_R);
    steps(t0, cur, cur_n);
    load_rows(cur, cur_n, t0 + 2 * CTC_R);
    steps(t0 + CTC_R, nxt, nxt_n);
  }

#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    const int s = (w * CPT + c) * 64 + lane;
    if (s == S - 1) fin[0] = prev[c];
    if (s == S - 2) fin[1] = prev[c];
  }
  __syncthreads();
  if (tid == 0) logp[b] = logaddexp_f(fin[0], fin[1]);
}

template <int CPT, bool MULTI>
void ctc_loss_launch(hipStream_t st, int threads, const float* scores, long long batch_stride, int ld, const int* labels,
                     int ld_lab, const int* t_len, const int* l_len, int blank, float* logp, const float* lse, int B, int T,
                     int L, int V) {
  hipLaunchKernelGGL((ctc_loss_kernel<CPT, MULTI>), dim3((unsigned)B), dim3((unsigned)threads), 0, st, scores, batch_stride,
                     ld, labels, ld_lab, t_len, l_len, blank, logp, lse, T, L, V);
}

int ctc_w64(int L) { return (2 * L + 1 + 63) / 64; }

// the operand checks that f5e_ctc_align and f5e_ctc_loss share (after their own null and range checks); name = "ctc_align" /
// "ctc_loss", need_bytes / align = what the entry point asks of its workspace
int ctc_check_common(const char* name, long long batch_stride, int ld, int ld_labels, int blank, const void* workspace,
                     unsigned long long workspace_bytes, unsigned long long need_bytes, int align, int B, int T, int L, int V) {
  F5E_REQUIRE(V >= 2 && blank >= 0 && blank < V, "%s: need V >= 2 and 0 <= blank < V", name);
  F5E_REQUIRE(ld >= V && ld_labels >= L && (B == 1 || batch_stride >= (long long)(T - 1) * ld + V),
              "%s: ld / ld_labels / batch_stride too small", name);
  F5E_REQUIRE(workspace_bytes >= need_bytes && ((uintptr_t)workspace & (uintptr_t)(align - 1)) == 0,
              "%s: workspace smaller than f5e_%s_workspace_bytes or not %d-byte aligned", name, name, align);
  return F5E_OK;
}

}  // namespace

int f5e_ctc_align_workspace_bytes(int B, int T, int L, unsigned long long* bytes_out_host) {
  F5E_REQUIRE(bytes_out_host, "ctc_align_workspace_bytes: null output");
  F5E_REQUIRE(B > 0 && T > 0 && T <= CTC_MAX_T && L > 0 && L <= CTC_MAX_L,
              "ctc_align_workspace_bytes: need B > 0, 0 < T <= %d and 0 < L <= %d", CTC_MAX_T, CTC_MAX_L);
  // two decision bits per state, rows padded to whole pairs of 64-bit words
  *bytes_out_host = (unsigned long long)B * (unsigned long long)T * (unsigned long long)ctc_w64(L) * 16ull;
  return F5E_OK;
}

int f5e_ctc_align(hipStream_t st, const float* scores, long long batch_stride, int ld, const int* labels, int ld_labels,
                  const int* t_len, const int* l_len, int blank, int* align, int* tok_start, int* tok_end, float* score,
                  void* workspace, unsigned long long workspace_bytes, int B, int T, int L, int V) {
  F5E_REQUIRE(scores && labels && t_len && l_len && align && workspace, "ctc_align: null operand");
  F5E_REQUIRE(B > 0 && T > 0 && T <= CTC_MAX_T && L > 0 && L <= CTC_MAX_L,
              "ctc_align: need B > 0, 0 < T <= %d and 0 < L <= %d", CTC_MAX_T, CTC_MAX_L);
  const int W64 = ctc_w64(L);
  if (int e = ctc_check_common("ctc_align", batch_stride, ld, ld_labels, blank, workspace, workspace_bytes,
                               (unsigned long long)B * T * W64 * 16ull, 8, B, T, L, V))
    return e;
  unsigned long long* dec = (unsigned long long*)workspace;
#define CTC_GO(CPT, MULTI, THREADS)                                                                                         \
  ctc_align_launch<CPT, MULTI>(st, THREADS, scores, batch_stride, ld, labels, ld_labels, t_len, l_len, blank, align,        \
                               tok_start, tok_end, score, dec, B, T, L, V, W64)
  F5E_SLOT_LADDER(W64, CTC_GO);
#undef CTC_GO
  F5E_LAUNCH_CHECK("ctc_align");
  return F5E_OK;
}

int f5e_ctc_loss_workspace_bytes(int B, int T, unsigned long long* bytes_out_host) {
  F5E_REQUIRE(bytes_out_host, "ctc_loss_workspace_bytes: null output");
  F5E_REQUIRE(B > 0 && T > 0 && T <= CTC_MAX_T, "ctc_loss_workspace_bytes: need B > 0 and 0 < T <= %d", CTC_MAX_T);
  *bytes_out_host = (unsigned long long)B * (unsigned long long)T * 4ull;   // the normaliser of every frame
  return F5E_OK;
}

int f5e_ctc_loss(hipStream_t st, const float* scores, long long batch_stride, int ld, const int* labels, int ld_labels,
                 const int* t_len, const int* l_len, int blank, float* logp, void* workspace,
                 unsigned long long workspace_bytes, int B, int T, int L, int V) {
  F5E_REQUIRE(scores && (labels || L == 0) && t_len && l_len && logp && workspace, "ctc_loss: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= CTC_MAX_T && L >= 0 && L <= CTC_MAX_L,
              "ctc_loss: need 0 < B <= 65535, 0 < T <= %d and 0 <= L <= %d", CTC_MAX_T, CTC_MAX_L);
  if (int e = ctc_check_common("ctc_loss", batch_stride, ld, ld_labels, blank, workspace, workspace_bytes,
                               (unsigned long long)B * T * 4ull, 4, B, T, L, V))
    return e;
  float* lse = (float*)workspace;
  hipLaunchKernelGGL(ctc_frame_lse_kernel, dim3((unsigned)((T + 3) / 4), (unsigned)B), dim3(256), 0, st, scores, batch_stride,
                     ld, t_len, lse, T, V);
  const int W64 = ctc_w64(L);
#define CTC_GO(CPT, MULTI, THREADS)                                                                                         \
  ctc_loss_launch<CPT, MULTI>(st, THREADS, scores, batch_stride, ld, labels, ld_labels, t_len, l_len, blank, logp, lse, B, \
                              T, L, V)
  F5E_SLOT_LADDER(W64, CTC_GO);
#undef CTC_GO
  F5E_LAUNCH_CHECK("ctc_loss");
  return F5E_OK;
}

int f5e_ctc_greedy(hipStream_t st, const float* scores, long long batch_stride, int ld, const int* t_len, int blank,
                   int pad_id, int* hyp, int* hyp_len, float* frame_logp, int B, int T, int V) {
  F5E_REQUIRE(scores && t_len && hyp && hyp_len, "ctc_greedy: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= CTC_MAX_T, "ctc_greedy: need 0 < B <= 65535 and 0 < T <= %d", CTC_MAX_T);
  F5E_REQUIRE(V >= 2 && blank >= 0 && blank < V && pad_id >= -1 && pad_id < V,
              "ctc_greedy: need V >= 2, 0 <= blank < V and -1 <= pad_id < V");
  F5E_REQUIRE(ld >= V && (B == 1 || batch_stride >= (long long)(T - 1) * ld + V), "ctc_greedy: ld / batch_stride too small");
  hipLaunchKernelGGL(ctc_frame_argmax_kernel, dim3((unsigned)((T + 3) / 4), (unsigned)B), dim3(256), 0, st, scores,
                     batch_stride, ld, hyp, frame_logp, T, V);
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3((unsigned)B), dim3(1024), 0, st, hyp, hyp_len, t_len, blank, pad_id, T);
  F5E_LAUNCH_CHECK("ctc_greedy");
  return F5E_OK;
}
