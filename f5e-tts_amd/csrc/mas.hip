// Monotonic alignment search (MAS): the Viterbi path through a [frames y][tokens x] log-likelihood matrix that starts at
// (0, 0), ends at (t_y - 1, t_x - 1) and moves by (+1, 0) or (+1, +1) per frame.  Replaces the host round trip of the
// reference (durpred/monotonic_align/__init__.py: D2H copy, a numba loop per utterance, H2D copy of the dense path) behind
// DiT.align_text_ppg (model/backbones/dit.py:309-331).
//
// One workgroup per sequence.  The recurrence Q[y][x] = L[y][x] + max(Q[y-1][x], Q[y-1][x-1]) is serial in y and parallel
// in x, so the depth is t_y steps whatever the mapping; what the mapping decides is the cost of one step:
//   * columns are dealt to waves in runs of 64 (slot c of wave w = columns (w * CPT + c) * 64 + lane): a row load is a
//     256-byte coalesced read per slot, and __ballot over a slot IS the 64-bit decision word of those columns;
//   * the previous row lives in REGISTERS (prev[CPT]); the diagonal neighbour comes from a one-lane wave rotate (DPP
//     wave_ror:1, a VALU move: no LDS crossbar on the dependent chain).  Lane 0 takes lane 63 of the slot before it, which is
//     the rotate's wrap-around of the previous slot;
//   * up to 256 tokens (CPT <= 4 slots) ONE wave carries the whole row: no LDS, no barrier.  Wider rows use up to 16 waves
//     of 4 slots; only the last column of each wave crosses waves, through a double-buffered LDS word and one barrier per row
//     (row y reads buffer (y - 1) & 1 and writes y & 1: a wave that is one row ahead writes the buffer nobody reads);
//   * logp rows are fetched MAS_R rows ahead into registers (the loads survive the barrier: plain loads, no LDS-DMA), with
//     the column index clamped into the band [lo(y), hi(y)], so lanes outside the band re-read an edge element (same cache
//     line) instead of fetching cells that are never used; no load sits under a per-lane branch;
//   * the backtrack is a chain of t_y dependent decisions.  It never touches Q again: the forward pass leaves one decision
//     bit per band cell ("step to x - 1 below this cell"), and wave 0 resolves 64 rows per round -- lane l fetches the two
//     words of row y0 - l that hold columns i - 63 .. i (the index moves by at most one per row), funnel-shifts them into a
//     64-bit window, and a 64-step scalar loop (v_readlane + s_lshr) walks the windows.  t_y / 64 dependent load rounds
//     instead of t_y.
// logp is only read.  Nothing is allocated or synchronised; the lengths are read on the device.
#include "f5e_common.h"

namespace {

constexpr float MAS_NEG = -1e9f;   // the reference's max_neg_val
constexpr int MAS_R = 8;           // rows of logp in flight per thread (x CPT registers, twice)
constexpr int MAS_MAX_TX = 4096;   // 16 waves x 4 slots x 64 columns

template <int CPT, bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void mas_kernel(const float* __restrict__ logp, long long batch_stride,
                                                                  int ld, const int* __restrict__ t_y_p,
                                                                  const int* __restrict__ t_x_p, int* __restrict__ tok_out,
                                                                  int* __restrict__ dur_out,
                                                                  unsigned long long* __restrict__ dec, int Ty, int Tx,
                                                                  int W64) {
  __shared__ float edge[2][16];        // Q of the last column of every wave, previous / current row
  __shared__ int tok_end[MULTI ? MAS_MAX_TX : CPT * 64];  // one past the last frame of every token (durations)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nt = blockDim.x;
  const int t_y = t_y_p[b], t_x = t_x_p[b];
  int* tok = tok_out + (long long)b * Ty;
  int* dur = dur_out ? dur_out + (long long)b * Tx : nullptr;
  // no monotonic path (or lengths beyond the matrix): -1 / 0 rows, defined and harmless
  const bool valid = t_x >= 1 && t_x <= Tx && t_y >= t_x && t_y <= Ty;
  for (int y = (valid ? t_y : 0) + tid; y < Ty; y += nt) tok[y] = -1;
  if (!valid) {  // workgroup-uniform
    if (dur)
      for (int x = tid; x < Tx; x += nt) dur[x] = 0;
    return;
  }

  const float* L = logp + (long long)b * batch_stride;
  unsigned long long* D = dec + (long long)b * Ty * W64;
  const int off = t_x - t_y;  // band of row y: max(0, off + y) .. min(t_x - 1, y)
  int xcol[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) xcol[c] = (w * CPT + c) * 64 + lane;

  float prev[CPT], cur[MAS_R][CPT], nxt[MAS_R][CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) prev[c] = 0.f;

  auto load_rows = [&](float (&dst)[MAS_R][CPT], int y0) {
#pragma unroll
    for (int r = 0; r < MAS_R; ++r) {
      const int y = min(y0 + r, t_y - 1);
      const int lo = max(0, off + y), hi = min(t_x - 1, y);
      const float* row = L + (long long)y * ld;
#pragma unroll
      for (int c = 0; c < CPT; ++c) dst[r][c] = row[min(max(xcol[c], lo), hi)];
    }
  };

  auto step = [&](int y, const float (&l)[CPT]) {
    const int lo = max(0, off + y), hi = min(t_x - 1, y);
    float e = MAS_NEG;
    // row y - 1 of the wave to the left; at y = 0 nothing has written it yet, and nothing uses it (only x = 0 is in band)
    if (MULTI && w > 0) e = edge[(y + 1) & 1][w - 1];
    float rot[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) rot[c] = wave_ror1(prev[c]);
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      const int x = xcol[c];
      const float dg = lane > 0 ? rot[c] : (c > 0 ? rot[c > 0 ? c - 1 : 0] : e);  // Q[y-1][x-1]
      const bool in = x >= lo && x <= hi;
      const float up = x < y ? prev[c] : MAS_NEG;
      const float diag = x > 0 ? dg : MAS_NEG;
      const float q = y == 0 ? l[c] : l[c] + fmaxf(up, diag);
      // the backtrack's test at (y, x): leave token x below this frame?  (x == y: it must; ties stay)
      const bool left = in && x > 0 && (x == y || prev[c] < dg);
      const unsigned long long word = __ballot(left);
      // a row of the scratch holds W64 = ceil(Tx / 64) words, fewer than the threads * CPT slots when Tx is small: the
      // wi < W64 test is what keeps the slots past the matrix from writing into the next row
      const int wi = w * CPT + c;
      if (lane == 0 && wi < W64 && wi * 64 <= hi && wi * 64 + 63 >= lo) D[(long long)y * W64 + wi] = word;
      prev[c] = in ? q : prev[c];
    }
    if (MULTI) {
      if (lane == 63) edge[y & 1][w] = prev[CPT - 1];
      __syncthreads();
    }
  };

  auto steps = [&](int y0, const float (&rows)[MAS_R][CPT]) {
#pragma unroll
    for (int r = 0; r < MAS_R; ++r)
      if (y0 + r < t_y) step(y0 + r, rows[r]);  // workgroup-uniform
  };
  load_rows(cur, 0);
  for (int y0 = 0; y0 < t_y; y0 += 2 * MAS_R) {  // the two register sets swap roles: no copies
    load_rows(nxt, y0 + MAS_R);
    steps(y0, cur);
    load_rows(cur, y0 + 2 * MAS_R);
    steps(y0 + MAS_R, nxt);
  }

  // The decision words are read back by wave 0 of this workgroup: a workgroup-scope release, then the barrier.  The
  // backtrack also FETCHES words of the caller's scratch that no wave wrote (words wholly outside a row's band, whatever the
  // scratch held); it only ever TESTS the bit of the cell the path is on, which lies in the band and so in a written word.
  __threadfence_block();
  __syncthreads();

  if (w == 0) {
    int i = t_x - 1;      // token of frame yb (wave-uniform)
    int above = t_x;      // token of frame yb + 1 (none above the last frame)
    for (int yb = t_y - 1; yb >= 0; yb -= 64) {
      const int y = yb - lane;
      const int cbase = i - 63;  // column of window bit 0; may be negative (those bits are never set or used)
      const int wa = cbase >> 6, s = cbase & 63;
      unsigned long long A = 0, Bw = 0;
      if (y >= 0) {
        const unsigned long long* drow = D + (long long)y * W64;
        if (wa >= 0) A = drow[wa];
        if (s != 0 && wa + 1 >= 0) Bw = drow[wa + 1];  // wa + 1 = i >> 6 < W64
      }
      const unsigned long long win = s ? (A >> s) | (Bw << (64 - s)) : A;
      const int win_lo = (int)(unsigned)win, win_hi = (int)(unsigned)(win >> 32);
      int p = 63, mine = 0;
#pragma unroll
      for (int l = 0; l < 64; ++l) {
        const unsigned long long wl = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(win_hi, l) << 32) |
                                      (unsigned)__builtin_amdgcn_readlane(win_lo, l);
        if (lane == l) mine = cbase + p;
        p -= (int)((wl >> p) & 1ull);
      }
      // frame y closes token `mine` when the frame above it belongs to another token
      int nb = __shfl_up(mine, 1, 64);
      if (lane == 0) nb = above;
      if (y >= 0) {
        tok[y] = mine;
        if (nb != mine) tok_end[min(max(mine, 0), t_x - 1)] = y + 1;
      }
      above = __builtin_amdgcn_readlane(mine, 63);
      i = cbase + p;
    }
  }
  if (dur) {
    __syncthreads();
    for (int x = tid; x < Tx; x += nt) dur[x] = x < t_x ? tok_end[x] - (x > 0 ? tok_end[x - 1] : 0) : 0;
  }
}

template <int CPT, bool MULTI>
void mas_launch(hipStream_t st, int threads, const float* logp, long long batch_stride, int ld, const int* t_y, const int* t_x,
                int* tok, int* dur, unsigned long long* dec, int B, int Ty, int Tx, int W64) {
  hipLaunchKernelGGL((mas_kernel<CPT, MULTI>), dim3((unsigned)B), dim3((unsigned)threads), 0, st, logp, batch_stride, ld, t_y,
                     t_x, tok, dur, dec, Ty, Tx, W64);
}

}  // namespace

int f5e_mas_workspace_bytes(int B, int Ty, int Tx, unsigned long long* bytes_out_host) {
  F5E_REQUIRE(bytes_out_host, "mas_workspace_bytes: null output");
  F5E_REQUIRE(B > 0 && Ty > 0 && Tx > 0 && Tx <= MAS_MAX_TX, "mas_workspace_bytes: need B, Ty > 0 and 0 < Tx <= %d", MAS_MAX_TX);
  // one decision bit per cell, rows padded to whole 64-bit words
  *bytes_out_host = (unsigned long long)B * (unsigned long long)Ty * (unsigned long long)((Tx + 63) / 64) * 8ull;
  return F5E_OK;
}

int f5e_mas_path(hipStream_t st, const float* logp, long long batch_stride, int ld, const int* t_y, const int* t_x,
                 int* token_of_frame, int* durations, void* workspace, unsigned long long workspace_bytes, int B, int Ty,
                 int Tx) {
  F5E_REQUIRE(logp && t_y && t_x && token_of_frame && workspace, "mas_path: null operand");
  F5E_REQUIRE(B > 0 && Ty > 0 && Tx > 0 && Tx <= MAS_MAX_TX, "mas_path: need B, Ty > 0 and 0 < Tx <= %d", MAS_MAX_TX);
  F5E_REQUIRE(ld >= Tx && (B == 1 || batch_stride >= (long long)(Ty - 1) * ld + Tx), "mas_path: ld / batch_stride too small");
  const int W64 = (Tx + 63) / 64;
  F5E_REQUIRE(workspace_bytes >= (unsigned long long)B * Ty * W64 * 8ull && ((uintptr_t)workspace & 7) == 0,
              "mas_path: workspace smaller than f5e_mas_workspace_bytes or not 8-byte aligned");
  unsigned long long* dec = (unsigned long long*)workspace;
#define MAS_GO(CPT, MULTI, THREADS) \
  mas_launch<CPT, MULTI>(st, THREADS, logp, batch_stride, ld, t_y, t_x, token_of_frame, durations, dec, B, Ty, Tx, W64)
  F5E_SLOT_LADDER(W64, MAS_GO);
#undef MAS_GO
  F5E_LAUNCH_CHECK("mas_path");
  return F5E_OK;
}
