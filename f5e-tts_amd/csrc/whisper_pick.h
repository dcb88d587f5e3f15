// The pick bodies of Whisper's greedy step, written once: f5e_greedy_pick / f5e_whisper_ts_pick / f5e_whisper_ts_rule
// (whisper.hip) run them on one logits row per workgroup, f5e_whisper_verify (whisper_append.hip) on U + 1 rows per decoder row.
// Every function here is called by all 256 threads of a workgroup; results are valid in thread 0.
#pragma once
#include "f5e_common.h"

constexpr int GP_MAX_V = 262144;   // one bit per class in LDS

// The suppressed classes as bits (the caller has zeroed `bits` and synchronises afterwards).
__device__ __forceinline__ void pick_mark_bits(unsigned* bits, const int* __restrict__ suppress, int n_sup,
                                               const int* __restrict__ begin_suppress, int n_beg, int V) {
  for (int i = threadIdx.x; i < n_sup + n_beg; i += 256) {
    const int v = i < n_sup ? suppress[i] : begin_suppress[i - n_sup];
    if (v >= 0 && v < V) atomicOr(&bits[v >> 5], 1u << (v & 31));
  }
}

// The first maximum of the classes that are not suppressed (0 for a row of NaN only).  rm, ra: 4 LDS words each.
__device__ __forceinline__ int greedy_pick_row(const float* __restrict__ row, const unsigned* bits, float* rm, int* ra, int V) {
  const int tid = threadIdx.x;
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
  }
  return arg;
}

// ---- timestamp rules (transformers' WhisperTimeStampLogitsProcessor, after the two suppress processors) ---------------------------
// Everything the processor bans is an interval: the text classes [0, eos) or [0, ts_begin), and the timestamps outside [lo, hi].
// One workgroup per row reads the logits once; a lane keeps, for the allowed timestamps and for the allowed text classes
// apart, a running maximum with its first index and the sum of exp(x - maximum).  The groups are folded across the wave by
// shuffles and across the waves through LDS in wave order, so the result does not depend on timing.  log-sum-exp(timestamps) >
// max(text) bans all text: the log-softmax normaliser of the processor is common to both sides and drops out.
struct TsRule {
  int kind, lo, hi;   // text ban: 0 none, 1 [0, eos), 2 [0, ts_begin); allowed timestamps [lo, hi] (lo > hi: none)
};

struct TsGroup {
  float m, s;         // maximum (-inf: no class), sum of exp(x - m)
  int a;              // lowest index of the maximum
};

// Four classes of a lane at once, v0 + 256 k (ascending): x[k] counts iff in[k].  One rescale of the sum per call, then four
// independent exponentials: the dependent chain of a lane is a quarter of the one-class-at-a-time form.
__device__ __forceinline__ void ts_group_add4(TsGroup& g, const float (&x)[4], const bool (&in)[4], int v0) {
  const float NEG = -__builtin_inff();
  float m4 = NEG;
#pragma unroll
  for (int k = 0; k < 4; ++k) m4 = in[k] ? fmaxf(m4, x[k]) : m4;
  if (!(m4 > NEG)) return;
  if (m4 > g.m) {                                 // '>' keeps the first maximum; the first class: 0 * exp(-inf) = 0
    g.s *= expf(g.m - m4);
    g.m = m4;
#pragma unroll
    for (int k = 3; k >= 0; --k)
      if (in[k] && x[k] == m4) g.a = v0 + 256 * k;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) g.s += in[k] ? expf(x[k] - g.m) : 0.f;
}

__device__ __forceinline__ void ts_group_merge(TsGroup& g, float om, float os, int oa) {
  const float M = fmaxf(g.m, om);
  const float fa = g.m == M ? 1.f : expf(g.m - M), fb = om == M ? 1.f : expf(om - M);   // -inf == -inf: no exp(NaN)
  g.s = g.s * fa + os * fb;
  if (om > g.m || (om == g.m && oa < g.a)) g.a = oa;
  g.m = M;
}

__device__ __forceinline__ void ts_group_wave(TsGroup& g) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(g.m, o, 64), os = __shfl_xor(g.s, o, 64);
    const int oa = __shfl_xor(g.a, o, 64);
    ts_group_merge(g, om, os, oa);
  }
}

// The state of a row from its generated tokens hist[0 .. len) (uniform over the workgroup; `slot` is one LDS word).
__device__ __forceinline__ TsRule ts_rule_of(const int* __restrict__ hist, int len, int V, int ts_begin, int max_initial,
                                             int* slot) {
  const int tid = threadIdx.x;
  if (tid == 0) *slot = -1;
  __syncthreads();
  int li = -1;
  for (int i = tid; i < len; i += 256)
    if (hist[i] >= ts_begin) li = i;
  if (li >= 0) atomicMax(slot, li);
  __syncthreads();
  li = *slot;
  TsRule d = {0, ts_begin, V - 1};
  const bool last_ts = len >= 1 && hist[len - 1] >= ts_begin;
  const bool pen_ts = len < 2 || hist[len - 2] >= ts_begin;
  if (last_ts) {
    if (pen_ts) d.lo = V;                         // a closed pair, or the opening timestamp: text has to follow
    else d.kind = 1;                              // text, timestamp: only [eos, ts_begin) and timestamps may follow
  }
  if (li >= 0) {                                  // timestamps do not decrease; only the one that closes a segment may repeat
    const int tl = min(hist[li], V - 1);
    d.lo = max(d.lo, last_ts && !pen_ts ? tl : tl + 1);
  }
  if (len == 0) {
    d.kind = 2;
    if (max_initial >= 0) d.hi = min(d.hi, ts_begin + min(max_initial, V));
  }
  return d;
}

// What the ruled step makes of one logits row (thread 0): the pick, the log-probability of the pick among the allowed classes
// (`has`: some class is allowed; otherwise arg = 0 and nothing is added), and whether the timestamps' mass bans all text.
struct TsPick {
  int arg;
  float logp;
  bool has, only_ts;
};

// rm, rs, ra: [2][4] LDS words each.  `bits` holds the suppressed classes; d the row's rule.
__device__ __forceinline__ TsPick ts_pick_row(const float* __restrict__ row, const unsigned* bits, const TsRule d, float (*rm)[4],
                                              float (*rs)[4], int (*ra)[4], int V, int eos, int no_ts) {
  const int tid = threadIdx.x, ts_begin = no_ts + 1;
  const float NEG = -__builtin_inff();
  TsGroup ts = {NEG, 0.f, WAVE_NONE}, tx = {NEG, 0.f, WAVE_NONE};
  const int text_from = d.kind == 2 ? ts_begin : d.kind == 1 ? eos : 0;
  for (int v0 = tid; v0 < V; v0 += 1024) {        // ascending per thread: '>' keeps the first maximum
    float x[4];
    bool is_ts[4], is_tx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = v0 + 256 * k;
      x[k] = v < V ? row[v] : NEG;
      const bool ok = v < V && !((bits[(v >> 5) & (GP_MAX_V / 32 - 1)] >> (v & 31)) & 1u) && v != no_ts && x[k] > NEG &&
                      x[k] < __builtin_inff();    // NaN, +-inf: no class
      is_ts[k] = ok && v >= ts_begin && v >= d.lo && v <= d.hi;
      is_tx[k] = ok && v < ts_begin && v >= text_from;
    }
    ts_group_add4(ts, x, is_ts, v0);
    ts_group_add4(tx, x, is_tx, v0);
  }
  ts_group_wave(ts);
  ts_group_wave(tx);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    rm[0][w] = ts.m, rs[0][w] = ts.s, ra[0][w] = ts.a;
    rm[1][w] = tx.m, rs[1][w] = tx.s, ra[1][w] = tx.a;
  }
  __syncthreads();
  TsPick out = {0, 0.f, false, false};
  if (tid == 0) {
    ts = {rm[0][0], rs[0][0], ra[0][0]}, tx = {rm[1][0], rs[1][0], ra[1][0]};
    for (int w = 1; w < 4; ++w) ts_group_merge(ts, rm[0][w], rs[0][w], ra[0][w]), ts_group_merge(tx, rm[1][w], rs[1][w], ra[1][w]);
    const float lse_ts = ts.m > NEG ? ts.m + logf(ts.s) : NEG;
    out.only_ts = lse_ts > tx.m;                  // the sum of the timestamps' probabilities beats every text class
    if (out.only_ts) tx = {NEG, 0.f, WAVE_NONE};
    const bool text_wins = tx.m >= ts.m && tx.a != WAVE_NONE;   // text ids lie below the timestamps: the lower index at a tie
    const int arg = text_wins ? tx.a : ts.a;
    const float xm = text_wins ? tx.m : ts.m;
    ts_group_merge(tx, ts.m, ts.s, ts.a);         // all allowed classes: tx.m = xm
    out.has = arg != WAVE_NONE;
    out.arg = out.has ? arg : 0;                  // nothing is allowed: 0
    if (out.has) out.logp = (xm - tx.m) - logf(tx.s);
  }
  return out;
}

// ---- the steps' bodies: one workgroup of 256 threads per row r = blockIdx.x ---------------------------------------------------
// The kernels of whisper.hip hand them the step's position p, the prompt length n0 and the begin-suppress count from their
// arguments, the device-position kernels of whisper_step.hip from the step record: one body, so the bits are the same.
// `n_beg` is 0 unless p + 1 == n0.

// Greedy: tokens[r][p + 1], last, done (0 -> 1).
__device__ __forceinline__ void greedy_pick_step(const float* __restrict__ logits, long long ld, const int* __restrict__ suppress,
                                                 int n_sup, const int* __restrict__ begin_suppress, int n_beg, int* tokens,
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
  pick_mark_bits(bits, suppress, n_sup, begin_suppress, n_beg, V);
  __syncthreads();
  const int arg = greedy_pick_row(logits + (size_t)r * ld, bits, rm, ra, V);
  if (tid == 0) {
    tokens[(size_t)r * ld_tok + p + 1] = arg;
    last[r] = arg;
    if (arg == eos) done[r] = 1;
  }
}

// The rows that are still open, counted by one workgroup of 256 threads (valid in thread 0).  red: 4 LDS words.
__device__ __forceinline__ int alive_count_rows(const int* __restrict__ done, int R, int* red) {
  int c = 0;
  for (int r = threadIdx.x; r < R; r += 256) c += done[r] ? 0 : 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// PICK: the ruled greedy step (tokens, last, done, sum_logp).  Otherwise the rule descriptor of the row goes to desc[r][0..4) for
// the beam's chunk kernel: kind, lo, hi, 0.  The generated tokens of row r are tokens[r][n0 .. p].
template <bool PICK>
__device__ __forceinline__ void ts_rule_step(const float* __restrict__ logits, long long ld, const int* __restrict__ suppress,
                                             int n_sup, const int* __restrict__ begin_suppress, int n_beg, int* tokens, int ld_tok,
                                             int* last, int* done, float* sum_logp, int* __restrict__ desc, int V, int p, int n0,
                                             int eos, int no_ts, int max_initial) {
  __shared__ unsigned bits[GP_MAX_V / 32];
  __shared__ float rm[2][4], rs[2][4];
  __shared__ int ra[2][4], slot;
  const int tid = threadIdx.x, r = blockIdx.x;
  if (PICK && done[r]) {                          // uniform over the workgroup
    if (tid == 0) tokens[(size_t)r * ld_tok + p + 1] = eos, last[r] = eos;
    return;
  }
  const int words = (V + 31) / 32, ts_begin = no_ts + 1;
  for (int i = tid; i < words; i += 256) bits[i] = 0u;
  const TsRule d = ts_rule_of(tokens + (size_t)r * ld_tok + n0, p + 1 - n0, V, ts_begin, max_initial, &slot);   // syncs twice
  pick_mark_bits(bits, suppress, n_sup, begin_suppress, n_beg, V);
  __syncthreads();
  const TsPick pk = ts_pick_row(logits + (size_t)r * ld, bits, d, rm, rs, ra, V, eos, no_ts);
  if (tid == 0) {
    if (!PICK) {
      int* dr = desc + (size_t)r * 4;
      dr[0] = pk.only_ts ? 2 : d.kind, dr[1] = d.lo, dr[2] = d.hi, dr[3] = 0;
      return;
    }
    if (pk.has) sum_logp[r] += pk.logp;
    tokens[(size_t)r * ld_tok + p + 1] = pk.arg;
    last[r] = pk.arg;
    if (pk.arg == eos) done[r] = 1;
  }
}

// ---- the sampled step under the rules (f5e_whisper_sample_pick) ---------------------------------------------------------------
// The noise is a function of counters only: class i takes word i & 3 of Philox4x32-10(counter = (i >> 2, step, serial, row_key),
// key = (seed_lo, seed_hi)), so a draw depends on neither the launch geometry nor the row's batch-mates.
__host__ __device__ inline void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&w)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long a = 0xD2511F53ull * c0, b = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(b >> 32) ^ c1 ^ k0, n2 = (unsigned)(a >> 32) ^ c3 ^ k1;
    c0 = n0, c1 = (unsigned)b, c2 = n2, c3 = (unsigned)a;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// g = -log(-log(u)), u = ((w >> 8) + 0.5) 2^-24.  n + 0.5 has 25 significant bits from n = 2^23 on and would round (to u = 1 at
// the top), so the upper half goes through 1 - u = ((2^24 - 1 - n) + 0.5) 2^-24, which is exact there, and log1p.
__device__ __forceinline__ float ws_gumbel(unsigned w) {
  const unsigned n = w >> 8;
  const float e = n < (1u << 23) ? -logf(((float)n + 0.5f) * 0x1p-24f) : -log1pf(-(((float)(0xffffffu - n) + 0.5f) * 0x1p-24f));
  return -logf(e);
}

struct WsDraw {
  float y, x;         // the largest perturbed value x / T + g and its raw logit
  int a;              // its lowest index (WAVE_NONE: no class)
};

__device__ __forceinline__ void ws_draw_merge(WsDraw& d, float oy, float ox, int oa) {
  if (oa != WAVE_NONE && (d.a == WAVE_NONE || oy > d.y || (oy == d.y && oa < d.a))) d = {oy, ox, oa};
}

__device__ __forceinline__ void ws_draw_wave(WsDraw& d) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float oy = __shfl_xor(d.y, o, 64), ox = __shfl_xor(d.x, o, 64);
    const int oa = __shfl_xor(d.a, o, 64);
    ws_draw_merge(d, oy, ox, oa);
  }
}

// ts_rule_step<true> with a draw for the argmax: the rules and the running log-sum-exp are decided on the raw logits (the
// temperature warper runs after the Whisper processors), the pick is the first maximum of x / T + g, kept for the timestamps and
// for the text apart because rule 6 is only known after the pass.  A lane owns 4 consecutive classes = one Philox block.
// no_ts < 0: no timestamp rules (every class is text, nothing but the suppressed classes is banned).
__device__ __forceinline__ void ts_sample_step(const float* __restrict__ logits, long long ld, const int* __restrict__ suppress,
                                               int n_sup, const int* __restrict__ begin_suppress, int n_beg, int* tokens, int ld_tok,
                                               int* last, int* done, float* sum_logp, int V, int p, int n0, int eos, int no_ts,
                                               int max_initial, float temperature, unsigned seed_lo, unsigned seed_hi,
                                               const int* __restrict__ row_key, const int* __restrict__ serial) {
  __shared__ unsigned bits[GP_MAX_V / 32];
  __shared__ float rm[2][4], rs[2][4], ry[2][4], rx[2][4];
  __shared__ int ra[2][4], slot;
  const int tid = threadIdx.x, r = blockIdx.x;
  if (done[r]) {                                  // uniform over the workgroup
    if (tid == 0) tokens[(size_t)r * ld_tok + p + 1] = eos, last[r] = eos;
    return;
  }
  const int words = (V + 31) / 32, ts_begin = no_ts >= 0 ? no_ts + 1 : V;
  for (int i = tid; i < words; i += 256) bits[i] = 0u;
  TsRule d = {0, V, V - 1};
  if (no_ts >= 0) d = ts_rule_of(tokens + (size_t)r * ld_tok + n0, p + 1 - n0, V, ts_begin, max_initial, &slot);   // syncs twice
  else __syncthreads();
  for (int i = tid; i < n_sup + n_beg; i += 256) {
    const int v = i < n_sup ? suppress[i] : begin_suppress[i - n_sup];
    if (v >= 0 && v < V) atomicOr(&bits[v >> 5], 1u << (v & 31));
  }
  __syncthreads();
  const float NEG = -__builtin_inff();
  const float* row = logits + (size_t)r * ld;
  const unsigned key_row = (unsigned)row_key[r], key_serial = (unsigned)serial[r];
  TsGroup ts = {NEG, 0.f, WAVE_NONE}, tx = {NEG, 0.f, WAVE_NONE};   // maximum and sum only: their index is not used here
  WsDraw dts = {NEG, NEG, WAVE_NONE}, dtx = {NEG, NEG, WAVE_NONE};
  const int text_from = d.kind == 2 ? ts_begin : d.kind == 1 ? eos : 0;
  for (int v0 = 4 * tid; v0 < V; v0 += 1024) {    // ascending per thread: '>' keeps the first maximum
    unsigned w[4];
    philox4x32_10((unsigned)(v0 >> 2), (unsigned)p, key_serial, key_row, seed_lo, seed_hi, w);
    float x[4];
    bool is_ts[4], is_tx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int v = v0 + k;
      x[k] = v < V ? row[v] : NEG;
      const bool ok = v < V && !((bits[(v >> 5) & (GP_MAX_V / 32 - 1)] >> (v & 31)) & 1u) && v != no_ts && x[k] > NEG &&
                      x[k] < __builtin_inff();    // NaN, +-inf: no class
      is_ts[k] = ok && v >= ts_begin && v >= d.lo && v <= d.hi;
      is_tx[k] = ok && v < ts_begin && v >= text_from;
      if (is_ts[k] || is_tx[k]) {
        const float y = x[k] / temperature + ws_gumbel(w[k]);
        WsDraw& dr = is_ts[k] ? dts : dtx;
        if (dr.a == WAVE_NONE || y > dr.y) dr = {y, x[k], v};
      }
    }
    ts_group_add4(ts, x, is_ts, v0);
    ts_group_add4(tx, x, is_tx, v0);
  }
  ts_group_wave(ts);
  ts_group_wave(tx);
  ws_draw_wave(dts);
  ws_draw_wave(dtx);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    rm[0][w] = ts.m, rs[0][w] = ts.s, ry[0][w] = dts.y, rx[0][w] = dts.x, ra[0][w] = dts.a;
    rm[1][w] = tx.m, rs[1][w] = tx.s, ry[1][w] = dtx.y, rx[1][w] = dtx.x, ra[1][w] = dtx.a;
  }
  __syncthreads();
  if (tid == 0) {
    ts = {rm[0][0], rs[0][0], 0}, tx = {rm[1][0], rs[1][0], 0};
    dts = {ry[0][0], rx[0][0], ra[0][0]}, dtx = {ry[1][0], rx[1][0], ra[1][0]};
    for (int w = 1; w < 4; ++w) {
      ts_group_merge(ts, rm[0][w], rs[0][w], 0), ts_group_merge(tx, rm[1][w], rs[1][w], 0);
      ws_draw_merge(dts, ry[0][w], rx[0][w], ra[0][w]), ws_draw_merge(dtx, ry[1][w], rx[1][w], ra[1][w]);
    }
    const float lse_ts = ts.m > NEG ? ts.m + logf(ts.s) : NEG;
    if (lse_ts > tx.m) tx = {NEG, 0.f, 0}, dtx = {NEG, NEG, WAVE_NONE};   // rule 6, on the raw logits: all text is banned
    ws_draw_merge(dtx, dts.y, dts.x, dts.a);      // the draw over all allowed classes
    ts_group_merge(tx, ts.m, ts.s, 0);            // their maximum and sum of exponentials at T = 1
    int arg = dtx.a;
    if (arg == WAVE_NONE) arg = 0;                // nothing is allowed
    else sum_logp[r] += (dtx.x - tx.m) - logf(tx.s);
    tokens[(size_t)r * ld_tok + p + 1] = arg;
    last[r] = arg;
    if (arg == eos) done[r] = 1;
  }
}
