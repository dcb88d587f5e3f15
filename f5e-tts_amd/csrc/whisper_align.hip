// Whisper word timestamps on the device (transformers' generation_whisper.py: _extract_token_timestamps, _median_filter,
// _dynamic_time_warping, which copy every cross-attention weight to the host and run a Python double loop per utterance):
// the cross-attention probabilities of a few "alignment heads", their normalisation and smoothing into a cost matrix, and
// dynamic time warping over it.  fp32 throughout; the rules are written out in include/f5e_abi.h.
//
//   f5e_cross_attn_probs_f32   the softmax of f5e_cross_attn_decode_f32 for the selected heads only, WRITTEN OUT (that kernel
//                              keeps it in LDS).  One workgroup per (row, selected head): the scores of all Tk keys go to LDS,
//                              one maximum and one sum per workgroup (folded over the waves in a fixed order), and only the
//                              first m_len columns are stored.  A separate launch: the decode kernel is not touched.
//   f5e_dtw_cost_f32           rules 2-4 in one launch.  A workgroup owns a tile of 64 columns of one utterance plus a halo of
//                              w / 2 on each side: phase 1 leaves mean and std of every (head, column) of the tile in LDS
//                              (two passes over the N rows, coalesced over the columns), phase 2 gives a thread one (row,
//                              column) at a time: per head the w normalised neighbours (reflected at the ends of the row), their
//                              median by rank counting (exact, no sort network to get wrong), the mean over the heads, the sign.
//   f5e_dtw_path               rules 5-7.  One workgroup per utterance, thread i owns lattice row i and walks it along the
//                              anti-diagonals d = i + j: cost[i][j - 1] is the thread's own last value (a register),
//                              cost[i - 1][j] is the neighbour's last value (LDS, double-buffered: one barrier per diagonal)
//                              and cost[i - 1][j - 1] is what the thread read from the neighbour one diagonal earlier (a
//                              register).  The C row of a thread is fetched 8 columns ahead into registers, so no global load
//                              sits on the chain of N + M - 1 barriers.  Two trace bits per cell, 16 cells to a word, one
//                              store per word, go to the caller's workspace (448 x 1500 cells are 168 KB: not LDS).  The
//                              backtrace is a chain of at most N + M dependent steps walked by ONE thread; it keeps the current
//                              trace word in a register, so it issues a dependent load only when the row or the word changes:
//                              at most N + M / 16 of them.
//
// Nothing here allocates, synchronises or reads back.  Lengths are DEVICE int32.  No atomics: the results are deterministic.
#include "f5e_common.h"

namespace {

constexpr int WA_MAX_TK = 4096;     // keys of a probs row (the limit of f5e_cross_attn_decode_f32)
constexpr int WA_MAX_N = 448;       // lattice rows = threads of the path kernel
constexpr int WA_MAX_M = 4096;      // lattice columns
constexpr int WA_MAX_SEL = 64;      // alignment heads
constexpr int WA_MAX_W = 15;        // median filter width
constexpr int WA_TILE = 64;         // columns per workgroup of the cost kernel
constexpr int WA_PF = 8;            // columns of C a path thread keeps in flight

// ---- probabilities of the selected heads ---------------------------------------------------------------------------------
template <int DK>
__global__ __launch_bounds__(256) void cross_attn_probs_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ K,
                                                               int ldk, const int* __restrict__ heads, const int* __restrict__ m_len,
                                                               int M_cap, float* __restrict__ probs,
                                                               long long stride_row, long long stride_sel, int rows_per_utt,
                                                               int Tk, int H, float scale) {
  __shared__ float s[WA_MAX_TK];
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int sel = blockIdx.x, r = blockIdx.y, u = r / rows_per_utt;
  const int h = heads[sel];
  const int m = min(m_len ? max(m_len[u], 0) : Tk, min(M_cap, Tk));
  if (h < 0 || h >= H || m == 0) return;          // workgroup-uniform: a head outside the layer writes nothing
  const float* qr = q + (size_t)r * ldq + h * DK;
  const float* Ku = K + (size_t)u * Tk * ldk + h * DK;
  f32x4 qv[DK / 4];
#pragma unroll
  for (int i = 0; i < DK / 4; ++i) qv[i] = *(const f32x4*)(qr + 4 * i);
  float mx = -__builtin_inff();
  for (int j = tid; j < Tk; j += 256) {
    const float* kr = Ku + (size_t)j * ldk;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < DK / 4; ++i) {
      const f32x4 kv = *(const f32x4*)(kr + 4 * i);
      acc += qv[i].x * kv.x + qv[i].y * kv.y + qv[i].z * kv.z + qv[i].w * kv.w;
    }
    acc *= scale;
    s[j] = acc;
    mx = fmaxf(mx, acc);
  }
  mx = wave_max(mx);
  if (lane == 0) red[0][w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
  float sum = 0.f;
  for (int j = tid; j < Tk; j += 256) {            // a thread rewrites only the entries it wrote
    const float e = expf(s[j] - mx);
    s[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) red[1][w] = sum;
  __syncthreads();
  sum = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  float* out = probs + (long long)r * stride_row + (long long)sel * stride_sel;
  for (int j = tid; j < m; j += 256) out[j] = s[j] / sum;
}

// ---- cost matrix: normalise over the rows, median along the columns, mean over the heads, negate ---------------------------
template <int W>
__global__ __launch_bounds__(256) void dtw_cost_kernel(const float* __restrict__ probs, int ld, const int* __restrict__ n_rows,
                                                       const int* __restrict__ m_len, float* __restrict__ C, int ldc, int n_sel,
                                                       int N_cap, int M_cap) {
  constexpr int PAD = W / 2, SPAN = WA_TILE + 2 * PAD;
  extern __shared__ float stat[];                 // [n_sel][SPAN][2] = mean, std
  const int tid = threadIdx.x, b = blockIdx.y, j0 = blockIdx.x * WA_TILE;
  const int n = min(max(n_rows[b], 0), N_cap), m = min(max(m_len[b], 0), M_cap);
  if (n == 0 || j0 >= m) return;                  // workgroup-uniform
  const bool filter = m > PAD;                    // the reference leaves rows of at most w / 2 columns unfiltered
  const float* P = probs + (size_t)b * n_sel * N_cap * ld;
  const float fn = (float)n;
  for (int e = tid; e < n_sel * SPAN; e += 256) {
    const int sidx = e / SPAN, c = e - sidx * SPAN, j = j0 - PAD + c;
    float mean = 0.f, sd = 0.f;
    if (j >= 0 && j < m) {
      const float* col = P + (size_t)sidx * N_cap * ld + j;
      float sum = 0.f;
      for (int t = 0; t < n; ++t) sum += col[(size_t)t * ld];
      mean = sum / fn;
      float var = 0.f;
      for (int t = 0; t < n; ++t) {
        const float dlt = col[(size_t)t * ld] - mean;
        var += dlt * dlt;
      }
      sd = sqrtf(var / fn);
    }
    stat[2 * e] = mean;
    stat[2 * e + 1] = sd;
  }
  __syncthreads();
  const int cols = min(WA_TILE, m - j0);
  // a column of zero deviation (every column when N = 1) gives z = 0, never NaN
  auto znorm = [](float p, float mean, float sd) { return sd > 0.f ? (p - mean) / sd : 0.f; };
  for (int e = tid; e < n * WA_TILE; e += 256) {
    const int t = e / WA_TILE, c = e - t * WA_TILE;
    if (c >= cols) continue;
    const int j = j0 + c;
    float acc = 0.f;
    for (int sidx = 0; sidx < n_sel; ++sidx) {
      const float* row = P + ((size_t)sidx * N_cap + t) * ld;
      const float* st = stat + 2 * sidx * SPAN;
      if (!filter) {
        acc += znorm(row[j], st[2 * (c + PAD)], st[2 * (c + PAD) + 1]);
        continue;
      }
      float z[W];
#pragma unroll
      for (int k = 0; k < W; ++k) {
        int jj = j + k - PAD;                     // reflect without repeating the edge; PAD < m, so one bounce is enough
        if (jj < 0) jj = -jj;
        if (jj >= m) jj = 2 * (m - 1) - jj;
        const int cc = jj - j0 + PAD;             // inside the tile's span: |jj - j| <= PAD
        z[k] = znorm(row[jj], st[2 * cc], st[2 * cc + 1]);
      }
      float med = z[0];
#pragma unroll
      for (int k = 0; k < W; ++k) {               // the element with exactly W / 2 elements before it in (value, index) order
        int rank = 0;
#pragma unroll
        for (int o = 0; o < W; ++o) rank += (z[o] < z[k] || (z[o] == z[k] && o < k)) ? 1 : 0;
        if (rank == PAD) med = z[k];
      }
      acc += med;
    }
    C[((size_t)b * N_cap + t) * ldc + j] = -(acc / (float)n_sel);
  }
}

// ---- dynamic time warping ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WA_MAX_N) void dtw_path_kernel(const float* __restrict__ C, int ldc, const int* __restrict__ n_rows,
                                                            const int* __restrict__ m_len, int* __restrict__ first_out,
                                                            unsigned* __restrict__ trace, int N_cap, int M_cap, int W16) {
  __shared__ float diag[2][WA_MAX_N];             // cost of row i (index i - 1) on the previous / the current anti-diagonal
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int n = n_rows[b], m = m_len[b];
  int* first = first_out + (size_t)b * N_cap;
  const bool valid = n >= 1 && n <= N_cap && m >= 1 && m <= M_cap;
  for (int t = (valid ? n : 0) + tid; t < N_cap; t += nt) first[t] = -1;
  if (!valid) return;                             // workgroup-uniform: lengths outside the matrix give a row of -1
  const float INF = __builtin_inff();
  const int i = tid + 1;                          // lattice row of this thread; rows beyond n idle (and read row n - 1 of C)
  const bool mine = tid < n;
  const float* Crow = C + ((size_t)b * N_cap + min(tid, n - 1)) * ldc;
  unsigned* Trow = trace + ((size_t)b * N_cap + min(tid, n - 1)) * W16;
  const int last_d = n + m;

  float cur[WA_PF], nxt[WA_PF];
  auto load = [&](float (&dst)[WA_PF], int d0) {
#pragma unroll
    for (int r = 0; r < WA_PF; ++r) dst[r] = Crow[min(max(d0 + r - i, 1), m) - 1];   // clamped: cells off the lattice are not used
  };
  float own = INF, dg = INF;                      // cost[i][j - 1] and cost[i - 1][j - 1] of the cell to come
  unsigned bits = 0u;
  auto step = [&](int d, float c) {
    const int j = d - i;
    if (mine && j >= 1 && j <= m) {
      // the neighbour was on column j one diagonal ago; row 0 is +inf except cost[0][0] = 0, column 0 is +inf
      const float c1 = i == 1 ? INF : diag[(d - 1) & 1][tid - 1];
      const float c0 = j == 1 ? (i == 1 ? 0.f : INF) : dg;
      const float c2 = j == 1 ? INF : own;
      float cc;
      unsigned t;
      if (c0 < c1 && c0 < c2) cc = c0, t = 0u;
      else if (c1 < c0 && c1 < c2) cc = c1, t = 1u;
      else cc = c2, t = 2u;                       // every tie goes left
      own = c + cc;                               // one fp32 addition
      dg = c1;
      diag[d & 1][tid] = own;
      const int k = (j - 1) & 15;
      bits |= t << (2 * k);
      if (k == 15 || j == m) {
        Trow[(j - 1) >> 4] = bits;
        bits = 0u;
      }
    }
    __syncthreads();                              // diagonal d is complete; d + 1 overwrites the buffer of d - 1, read before this
  };
  auto steps = [&](int d0, const float (&c)[WA_PF]) {
#pragma unroll
    for (int r = 0; r < WA_PF; ++r)
      if (d0 + r <= last_d) step(d0 + r, c[r]);   // workgroup-uniform
  };
  load(cur, 2);
  for (int d0 = 2; d0 <= last_d; d0 += 2 * WA_PF) {   // the two register sets swap roles: no copies
    load(nxt, d0 + WA_PF);
    steps(d0, cur);
    load(cur, d0 + 2 * WA_PF);
    steps(d0 + WA_PF, nxt);
  }

  // the trace words are read back by thread 0 of this workgroup: a workgroup-scope release, then the barrier
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {
    const unsigned* T = trace + (size_t)b * N_cap * W16;
    int bi = n, bj = m, wi = -1, wrow = -1;
    unsigned word = 0u;
    while (bi > 0 || bj > 0) {
      unsigned t;
      if (bi == 0) t = 2u;                        // row 0 forces left, column 0 forces up (neither happens with finite costs)
      else if (bj == 0) t = 1u;
      else {
        const int wj = (bj - 1) >> 4;
        if (wj != wi || bi != wrow) word = T[(size_t)(bi - 1) * W16 + wj], wi = wj, wrow = bi;
        t = (word >> (2 * ((bj - 1) & 15))) & 3u;
      }
      if (bi > 0 && t != 2u) first[bi - 1] = bj - 1;   // the path leaves row bi here: the column at which it entered it
      if (t == 0u) --bi, --bj;
      else if (t == 1u) --bi;
      else --bj;
    }
  }
}

}  // namespace

extern "C" int f5e_cross_attn_probs_f32(hipStream_t st, const float* q, int ldq, const float* k, int ldk, const int* heads,
                                        int n_sel, const int* m_len, int M_cap, float* probs, long long stride_row,
                                        long long stride_sel, int R, int rows_per_utt, int Tk, int H, int dk, float scale) {
  F5E_REQUIRE(q && k && heads && probs, "cross_attn_probs_f32: null operand");
  F5E_REQUIRE(R > 0 && R <= 65535 && H > 0 && H <= 65535 && rows_per_utt > 0 && R % rows_per_utt == 0,
              "cross_attn_probs_f32: need 0 < R, H <= 65535 and R a multiple of rows_per_utt (R=%d rows_per_utt=%d)", R,
              rows_per_utt);
  F5E_REQUIRE(n_sel > 0 && n_sel <= 65535, "cross_attn_probs_f32: need 0 < n_sel <= 65535 (got %d)", n_sel);
  if (dk != 16 && dk != 32 && dk != 64 && dk != 128) {
    f5e_set_error("cross_attn_probs_f32: head dim must be 16, 32, 64 or 128 (got %d)", dk);
    return F5E_ERR_UNSUPPORTED;
  }
  F5E_REQUIRE(Tk > 0 && Tk <= WA_MAX_TK, "cross_attn_probs_f32: need 0 < Tk <= %d", WA_MAX_TK);
  const long long HD = (long long)H * dk;
  F5E_REQUIRE(ldq >= HD && ldk >= HD, "cross_attn_probs_f32: a row stride is smaller than H * dk");
  F5E_REQUIRE(ldq % 4 == 0 && ldk % 4 == 0 && (((uintptr_t)q | (uintptr_t)k) & 15) == 0,
              "cross_attn_probs_f32: q / k strides must be multiples of 4 floats, q and k 16-byte aligned");
  F5E_REQUIRE(stride_row >= 0 && stride_sel >= 0 && M_cap >= 1, "cross_attn_probs_f32: negative output stride or M_cap < 1");
  const dim3 grid((unsigned)n_sel, (unsigned)R), block(256);
#define F5E_XP_LAUNCH(DK)                                                                                                    \
  hipLaunchKernelGGL(cross_attn_probs_kernel<DK>, grid, block, 0, st, q, ldq, k, ldk, heads, m_len, M_cap, probs, stride_row, \
                     stride_sel, rows_per_utt, Tk, H, scale)
  switch (dk) {
    case 16: F5E_XP_LAUNCH(16); break;
    case 32: F5E_XP_LAUNCH(32); break;
    case 64: F5E_XP_LAUNCH(64); break;
    default: F5E_XP_LAUNCH(128); break;
  }
#undef F5E_XP_LAUNCH
  F5E_LAUNCH_CHECK("cross_attn_probs_f32");
  return F5E_OK;
}

extern "C" int f5e_dtw_cost_f32(hipStream_t st, const float* probs, int ld, const int* n_rows, const int* m_len, float* C,
                                int ldc, int B, int n_sel, int N_cap, int M_cap, int width) {
  F5E_REQUIRE(probs && n_rows && m_len && C, "dtw_cost_f32: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && N_cap >= 1 && N_cap <= WA_MAX_N && M_cap >= 1 && M_cap <= WA_MAX_M,
              "dtw_cost_f32: need 0 < B <= 65535, 1 <= N_cap <= %d, 1 <= M_cap <= %d (B=%d N_cap=%d M_cap=%d)", WA_MAX_N, WA_MAX_M,
              B, N_cap, M_cap);
  F5E_REQUIRE(ld >= M_cap && ldc >= M_cap, "dtw_cost_f32: a row stride is smaller than M_cap");
  if (n_sel < 1 || n_sel > WA_MAX_SEL || width < 1 || width > WA_MAX_W || width % 2 == 0) {
    f5e_set_error("dtw_cost_f32: built for 1 .. %d heads and an odd filter width of 1 .. %d (got %d, %d)", WA_MAX_SEL, WA_MAX_W,
                  n_sel, width);
    return F5E_ERR_UNSUPPORTED;
  }
  const dim3 grid((unsigned)((M_cap + WA_TILE - 1) / WA_TILE), (unsigned)B), block(256);
  const size_t lds = (size_t)n_sel * (WA_TILE + 2 * (width / 2)) * 2 * sizeof(float);   // at most 39 KB
#define F5E_DC_LAUNCH(W) \
  hipLaunchKernelGGL(dtw_cost_kernel<W>, grid, block, lds, st, probs, ld, n_rows, m_len, C, ldc, n_sel, N_cap, M_cap)
  switch (width) {
    case 1: F5E_DC_LAUNCH(1); break;
    case 3: F5E_DC_LAUNCH(3); break;
    case 5: F5E_DC_LAUNCH(5); break;
    case 7: F5E_DC_LAUNCH(7); break;
    case 9: F5E_DC_LAUNCH(9); break;
    case 11: F5E_DC_LAUNCH(11); break;
    case 13: F5E_DC_LAUNCH(13); break;
    default: F5E_DC_LAUNCH(15); break;
  }
#undef F5E_DC_LAUNCH
  F5E_LAUNCH_CHECK("dtw_cost_f32");
  return F5E_OK;
}

extern "C" int f5e_dtw_workspace_bytes(int B, int N_cap, int M_cap, unsigned long long* bytes_out_host) {
  F5E_REQUIRE(bytes_out_host, "dtw_workspace_bytes: null output");
  F5E_REQUIRE(B > 0 && B <= 65535 && N_cap >= 1 && N_cap <= WA_MAX_N && M_cap >= 1 && M_cap <= WA_MAX_M,
              "dtw_workspace_bytes: need 0 < B <= 65535, 1 <= N_cap <= %d, 1 <= M_cap <= %d", WA_MAX_N, WA_MAX_M);
  // two trace bits per cell, rows padded to whole 32-bit words
  *bytes_out_host = (unsigned long long)B * (unsigned long long)N_cap * (unsigned long long)((M_cap + 15) / 16) * 4ull;
  return F5E_OK;
}

extern "C" int f5e_dtw_path(hipStream_t st, const float* C, int ldc, const int* n_rows, const int* m_len, int* first,
                            void* workspace, unsigned long long workspace_bytes, int B, int N_cap, int M_cap) {
  F5E_REQUIRE(C && n_rows && m_len && first && workspace, "dtw_path: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && N_cap >= 1 && M_cap >= 1, "dtw_path: need 0 < B <= 65535, N_cap >= 1, M_cap >= 1 (B=%d)", B);
  if (N_cap > WA_MAX_N || M_cap > WA_MAX_M) {
    f5e_set_error("dtw_path: built for at most %d rows and %d columns (got %d, %d)", WA_MAX_N, WA_MAX_M, N_cap, M_cap);
    return F5E_ERR_UNSUPPORTED;
  }
  F5E_REQUIRE(ldc >= M_cap, "dtw_path: ldc is smaller than M_cap");
  const int W16 = (M_cap + 15) / 16;
  F5E_REQUIRE(workspace_bytes >= (unsigned long long)B * N_cap * W16 * 4ull && ((uintptr_t)workspace & 3) == 0,
              "dtw_path: workspace smaller than f5e_dtw_workspace_bytes or not 4-byte aligned");
  const int threads = (N_cap + 63) / 64 * 64;
  hipLaunchKernelGGL(dtw_path_kernel, dim3((unsigned)B), dim3((unsigned)threads), 0, st, C, ldc, n_rows, m_len, first,
                     (unsigned*)workspace, N_cap, M_cap, W16);
  F5E_LAUNCH_CHECK("dtw_path");
  return F5E_OK;
}
