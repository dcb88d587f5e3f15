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
