// CTC prefix beam search on the device (f5e_ctc_beam; fed chunk by chunk with a caller-owned state: f5e_ctc_beam_state_init /
// f5e_ctc_beam_chunk, the same frame body, described where the state is), the per-row target log-probability of the rescoring sum
// (f5e_token_logp) and the row log-softmax of forward_attention_decoder (f5e_log_softmax_rows).  Replaces the reference's
// host route ASRModel._ctc_prefix_beam_search (ppg/asr_model.py:461-546: a Python loop over frames, symbols and prefixes
// with an .item() per symbol, a dict and a sort per frame, asserted to batch 1) and the D2H of [N, U, V] log-probabilities
// plus the Python double loop of attention_rescoring (:651-677).
//
// ---- f5e_ctc_beam, two launches.
// Launch 1 (ctc_beam_topk_kernel), one wave per frame t < t_len: the first prune.  K rounds of wave argmax over the V scores
// of the row; round r takes the largest element that sorts AFTER round r-1's winner in the order (value descending, class
// index ascending), so nothing is marked and equal values come out lowest class first.  Round 0's winner is the row maximum
// m: log p(v) = (x[v] - m) - log1p(sum over the other classes of exp(x - m)), the form of f5e_ctc_greedy, so raw logits and
// log-probabilities give the same numbers.  K (class, log p) pairs per frame go to the workspace: the serial launch reads K
// pairs per frame instead of V floats.
//
// Launch 2 (ctc_beam_search_kernel), one workgroup per sequence, one thread per candidate of a frame: K "stay" candidates
// (beam entry p keeps its prefix) and K x K "extend" candidates (beam entry p, symbol j of the frame's top K).  The beam
// (node, parent node, last token, length, hash, pb, pnb per entry, best first) lives in LDS, double buffered.  Per frame:
//   1. cell (p, j) with symbol s: blank -> the stay candidate's pb = logaddexp(pb + ps, pnb + ps); s = last token of p ->
//      the stay candidate's repeat term pnb + ps and the extension value pb + ps; otherwise the extension value
//      logaddexp(pb + ps, pnb + ps).  The extension p + (s) is looked up among the beam entries (at most one can be that
//      prefix); found -> its value is handed to that entry's stay candidate (a merge), else the cell is a candidate itself;
//   2. stay candidate p: pb = blank term, pnb = logaddexp(repeat term, merged term); it exists iff one of the three does
//      (the reference's dict holds a prefix only once something touched it);
//   3. ranking by counting: a candidate's rank is the number of candidates that beat it (total descending, candidate index
//      ascending); ranks < K form the next beam, a kept new prefix taking trie node 1 + t K + rank.  No atomics on memory, no
//      sort.
// Prefix identity is exact: a prefix is a trie node (parent node, token) in the workspace; "q is p + (s)" holds at once when
// parent(q) = node(p) and last(q) = s.  A prefix that left the beam and was created again owns a second node while a
// descendant of the first may still be alive, so a q with equal length, last token and 32-bit prefix hash but another parent
// is compared token by token along both parent chains (rare; the hash only filters).
// The backtrace runs K lanes, one hypothesis each, along the parent pointers.
#include "f5e_common.h"

namespace {

constexpr int BEAM_MAX_K = 16;
constexpr int BEAM_MAX_T = 16384;
constexpr int BEAM_MAX_C = BEAM_MAX_K + BEAM_MAX_K * BEAM_MAX_K;   // candidates per frame

// The search keeps this spelling beside logaddexp_f (f5e_common.h): the two agree bit for bit on every non-NaN input, but the
// early return skips the transcendentals of the many (-inf, -inf) candidates, and with the shared form f5e_ctc_beam measured
// 0.4-0.7 % slower.  (On a NaN operand this one drops the NaN; the search's operands are NaN only for a row of scores that
// holds NaN or +inf or nothing but -inf.)
__device__ __forceinline__ float beam_logaddexp(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  if (!(m > -__builtin_inff())) return m;   // both -inf
  return m + log1pf(expf(n - m));
}

__device__ __forceinline__ unsigned hash_step(unsigned h, int tok) {
  h ^= (unsigned)tok + 0x9e3779b9u + (h << 6) + (h >> 2);
  return h * 0x85ebca6bu;
}

// one wave per frame: top K classes (value descending, class ascending) and their log-probabilities
__global__ __launch_bounds__(256) void ctc_beam_topk_kernel(const float* __restrict__ scores, long long batch_stride, int ld,
                                                             const int* __restrict__ t_len_p, int* __restrict__ top_id,
                                                             float* __restrict__ top_lp, int T, int T_ws, int V, int K) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  const int t_len = t_len_p[b];
  if (t >= T || t_len > T || t >= t_len) return;   // wave-uniform
  const float* row = scores + (long long)b * batch_stride + (long long)t * ld;
  const float NEG = -__builtin_inff();
  float pv = __builtin_inff(), m0 = 0.f, lse = 0.f;
  int pi = -1;
  for (int r = 0; r < K; ++r) {
    float m = NEG;
    int arg = WAVE_NONE;
    for (int v = lane; v < V; v += 64) {
      const float x = row[v];
      const bool after = x < pv || (x == pv && v > pi);
      if (after && (arg == WAVE_NONE || x > m)) m = x, arg = v;   // ascending v per lane: the first maximum stays
    }
    wave_argmax(m, arg);
    if (r == 0) {
      float sum = 0.f;
      for (int v = lane; v < V; v += 64) sum += v == arg ? 0.f : expf(row[v] - m);
      lse = log1pf(wave_sum(sum));
      m0 = m;
    }
    if (lane == 0) {
      const long long o = ((long long)b * T_ws + t) * K + r;   // T_ws >= T: the sequence's share of the scratch
      const bool none = arg == WAVE_NONE;   // fewer than K comparable values (NaN in the row)
      top_id[o] = none ? -1 : arg;
      top_lp[o] = none ? NEG : (m - m0) - lse;
    }
    pv = m, pi = arg;
  }
}

// the beam of one sequence and one frame's candidate bookkeeping, in LDS
struct BeamLds {
  int node[2][BEAM_MAX_K], par[2][BEAM_MAX_K], last[2][BEAM_MAX_K], len[2][BEAM_MAX_K];
  unsigned hash[2][BEAM_MAX_K];
  float pb[2][BEAM_MAX_K], pnb[2][BEAM_MAX_K];
  int nb[2];
  float s_blank[BEAM_MAX_K], s_rep[BEAM_MAX_K], s_merge[BEAM_MAX_K];
  int f_blank[BEAM_MAX_K], f_rep[BEAM_MAX_K], f_merge[BEAM_MAX_K];
  __attribute__((aligned(16))) unsigned key[BEAM_MAX_C];
};

// -1 / -1 / -inf rows of one sequence (workgroup-uniform call)
__device__ __forceinline__ void beam_fail_rows(int* H, int ld_hyp, int* hyp_len, float* score, int b, int K) {
  const int c = threadIdx.x, nt = blockDim.x;
  for (long long i = c; i < (long long)K * ld_hyp; i += nt) H[i] = -1;
  if (c < K) hyp_len[(long long)b * K + c] = -1, score[(long long)b * K + c] = -__builtin_inff();
}

// clears the per-frame flags and keys; the caller fills the beam of parity (t0 & 1) and then meets a barrier
__device__ __forceinline__ void beam_clear(BeamLds& L) {
  const int c = threadIdx.x, nt = blockDim.x;
  if (c < BEAM_MAX_K) L.f_blank[c] = L.f_rep[c] = L.f_merge[c] = 0;
  for (int i = c; i < BEAM_MAX_C; i += nt) L.key[i] = 0;
}

// THE frame body, shared by the whole-utterance search and the resumable one: n frames whose first is the sequence's
// absolute frame t0.  top_id / top_lp hold the first prune of these n frames (frame i at [i K, i K + K)); the trie arrays are
// the sequence's own and are indexed by absolute frame.  The beam of frame t0 is in the LDS buffer of parity t0 & 1 (a barrier
// lies between its writes and this call); the beam after the last frame is left in the buffer of parity (t0 + n) & 1, behind
// a barrier.
__device__ __forceinline__ void beam_frames(BeamLds& L, const int* __restrict__ top_id, const float* __restrict__ top_lp,
                                            int* trie_par, int* trie_tok, int t0, int n, int blank, int K) {
  const int c = threadIdx.x;
  const int NC = K + K * K, NC4 = (NC + 3) & ~3;
  const float NEG = -__builtin_inff();
  const bool is_stay = c < K, is_cell = c >= K && c < NC;
  const int p = is_cell ? (c - K) / K : c, j = is_cell ? (c - K) % K : 0;
  int s = -1;
  float ps = NEG;
  if (is_cell && n > 0) s = top_id[j], ps = top_lp[j];

  for (int i = 0; i < n; ++i) {
    const int t = t0 + i;
    const int cur = t & 1, nxt = cur ^ 1;
    const int nb = L.nb[cur];
    // ---- 1. the cells
    float val = NEG, n_pb = NEG, n_pnb = NEG;
    int node_p = 0, len_p = 0;
    unsigned hash_n = 0, k = 0;
    if (c == 0) L.nb[nxt] = 0;
    if (is_cell && p < nb && s >= 0) {
      node_p = L.node[cur][p], len_p = L.len[cur][p];
      const int last_p = L.last[cur][p];
      const float pb = L.pb[cur][p], pnb = L.pnb[cur][p];
      const float both = beam_logaddexp(pb + ps, pnb + ps);
      if (s == blank) {
        L.s_blank[p] = both, L.f_blank[p] = 1;
      } else {
        if (s == last_p) L.s_rep[p] = pnb + ps, L.f_rep[p] = 1;
        val = s == last_p ? pb + ps : both;
        hash_n = hash_step(L.hash[cur][p], s);
        int q = -1;
        for (int e = 0; e < nb; ++e) {
          if (L.last[cur][e] != s || L.len[cur][e] != len_p + 1) continue;
          int x = L.par[cur][e], y = node_p;
          if (x != y && L.hash[cur][e] != hash_n) continue;
          bool same = true;   // both chains hold len_p tokens: they meet at a common node (the root at the latest) or differ
          while (x != y) {
            if (x <= 0 || y <= 0 || trie_tok[x - 1] != trie_tok[y - 1]) {
              same = false;
              break;
            }
            x = trie_par[x - 1], y = trie_par[y - 1];
          }
          if (same) q = e;
        }
        if (q >= 0) L.s_merge[q] = val, L.f_merge[q] = 1;   // one writer: q's prefix minus its last token is one beam entry
        else k = rank_key(val);
      }
    }
    if (is_cell) L.key[c] = k;
    int s_next = -1;
    float ps_next = NEG;
    if (is_cell && i + 1 < n) s_next = top_id[(i + 1) * K + j], ps_next = top_lp[(i + 1) * K + j];
    __syncthreads();
    // ---- 2. the stay candidates
    if (is_stay) {
      k = 0;
      if (c < nb && (L.f_blank[c] | L.f_rep[c] | L.f_merge[c])) {
        n_pb = L.f_blank[c] ? L.s_blank[c] : NEG;
        n_pnb = beam_logaddexp(L.f_rep[c] ? L.s_rep[c] : NEG, L.f_merge[c] ? L.s_merge[c] : NEG);
        k = rank_key(beam_logaddexp(n_pb, n_pnb));
      }
      L.key[c] = k;
    }
    __syncthreads();
    // ---- 3. rank by counting; ranks < K are the next beam
    if (c < BEAM_MAX_K) L.f_blank[c] = L.f_rep[c] = L.f_merge[c] = 0;
    if (k != 0) {
      int rank = 0;
      for (int e = 0; e < NC4; e += 4) {
        const uint4 o = *(const uint4*)&L.key[e];
        rank += (o.x > k || (o.x == k && e < c)) + (o.y > k || (o.y == k && e + 1 < c)) +
                (o.z > k || (o.z == k && e + 2 < c)) + (o.w > k || (o.w == k && e + 3 < c));
      }
      if (rank < K) {
        atomicAdd(&L.nb[nxt], 1);
        if (is_stay) {
          L.node[nxt][rank] = L.node[cur][c], L.par[nxt][rank] = L.par[cur][c], L.last[nxt][rank] = L.last[cur][c];
          L.len[nxt][rank] = L.len[cur][c], L.hash[nxt][rank] = L.hash[cur][c];
          L.pb[nxt][rank] = n_pb, L.pnb[nxt][rank] = n_pnb;
        } else {
          const int slot = t * K + rank;   // < T K: inside the sequence's share of the trie
          L.node[nxt][rank] = 1 + slot, L.par[nxt][rank] = node_p, L.last[nxt][rank] = s;
          L.len[nxt][rank] = len_p + 1, L.hash[nxt][rank] = hash_n;
          L.pb[nxt][rank] = NEG, L.pnb[nxt][rank] = val;
          trie_par[slot] = node_p, trie_tok[slot] = s;
        }
      }
    }
    s = s_next, ps = ps_next;
    // the trie is read back by other threads of this workgroup: a workgroup-scope release, then the barrier
    __threadfence_block();
    __syncthreads();
  }
}

// the backtrace of the beam in the LDS buffer `fin`: lane q walks hypothesis q along the parent pointers; the -1 padding is
// dealt over the whole workgroup.  Reads the beam and the trie, writes the three outputs only.
__device__ __forceinline__ void beam_backtrace(const BeamLds& L, int fin, const int* trie_par, const int* trie_tok, int* H,
                                               int ld_hyp, int* hyp_len, float* score, int b, int K) {
  const int c = threadIdx.x, nt = blockDim.x;
  const int nb = min(L.nb[fin], K);
  for (int q = 0; q < K; ++q) {
    const int from = q < nb ? min(L.len[fin][q], ld_hyp) : 0;
    for (int i = from + c; i < ld_hyp; i += nt) H[(long long)q * ld_hyp + i] = -1;
  }
  if (c < K) {
    int len = -1;
    float sc = -__builtin_inff();
    if (c < nb) {
      len = L.len[fin][c];
      sc = beam_logaddexp(L.pb[fin][c], L.pnb[fin][c]);
      int node = L.node[fin][c];
      for (int pos = len - 1; pos >= 0 && node > 0; --pos) {
        if (pos < ld_hyp) H[(long long)c * ld_hyp + pos] = trie_tok[node - 1];
        node = trie_par[node - 1];
      }
    }
    hyp_len[(long long)b * K + c] = len;
    score[(long long)b * K + c] = sc;
  }
}

__global__ __launch_bounds__(320) void ctc_beam_search_kernel(const int* __restrict__ top_id, const float* __restrict__ top_lp,
                                                               int* trie_par, int* trie_tok,
                                                               const int* __restrict__ t_len_p, int blank,
                                                               int* __restrict__ hyp, int ld_hyp, int* __restrict__ hyp_len,
                                                               float* __restrict__ score, int T, int K) {
  __shared__ BeamLds L;
  const int b = blockIdx.x, c = threadIdx.x;
  const int t_len = t_len_p[b];
  int* H = hyp + (long long)b * K * ld_hyp;
  if (t_len < 0 || t_len > T) {   // workgroup-uniform: -1 / -inf rows, defined and harmless
    beam_fail_rows(H, ld_hyp, hyp_len, score, b, K);
    return;
  }
  const long long base = (long long)b * T * K;
  top_id += base, top_lp += base, trie_par += base, trie_tok += base;
  beam_clear(L);
  if (c == 0) {   // the empty prefix: the trie's root, node 0
    L.node[0][0] = 0, L.par[0][0] = -1, L.last[0][0] = -1, L.len[0][0] = 0, L.hash[0][0] = 0;
    L.pb[0][0] = 0.f, L.pnb[0][0] = -__builtin_inff();
    L.nb[0] = 1;
  }
  __syncthreads();
  beam_frames(L, top_id, top_lp, trie_par, trie_tok, 0, t_len, blank, K);
  beam_backtrace(L, t_len & 1, trie_par, trie_tok, H, ld_hyp, hyp_len, score, b, K);
}

// ---- the resumable search (f5e_ctc_beam_state_init / f5e_ctc_beam_chunk).  The state, in 4-byte words:
//   [0, 16)                         magic, B, T_cap, chunk_cap, beam (what state_init was given; a chunk call with another
//                                   geometry, or on a state never initialised, fails every sequence and writes no state)
//   16 + b 128 + [0, 128)           sequence b: frames consumed (-1 = dead), beam entries, then node / parent / last token /
//                                   length / hash / pb / pnb, BEAM_MAX_K words each
//   then  trie parent [B][T_cap][K], trie token [B][T_cap][K], top-K class [B][chunk_cap][K], top-K log p [B][chunk_cap][K].
constexpr int STATE_MAGIC = 0x43544362;   // "CTCb"
constexpr int STATE_HEAD = 16, STATE_SEQ = 128;
constexpr int STATE_MAX_T = 1 << 20;      // (T_cap + 1) K stays far below 2^31: node numbers are ints

__host__ __device__ inline unsigned long long state_words(long long B, long long T_cap, long long chunk_cap, long long K) {
  return (unsigned long long)(STATE_HEAD + B * STATE_SEQ + 2 * B * T_cap * K + 2 * B * chunk_cap * K);
}

// one workgroup of STATE_SEQ threads per sequence: every word of the two headers is written, nothing is read
__global__ __launch_bounds__(STATE_SEQ) void ctc_beam_state_init_kernel(int* state, int B, int T_cap, int chunk_cap, int K) {
  const int b = blockIdx.x, c = threadIdx.x;
  if (b == 0 && c < STATE_HEAD) {
    const int head[5] = {STATE_MAGIC, B, T_cap, chunk_cap, K};
    state[c] = c < 5 ? head[c] : 0;
  }
  int v = 0;                                               // consumed 0; entry 0 = the empty prefix, node 0, (0, -inf)
  if (c == 1) v = 1;                                       // one beam entry
  if (c == 2 + BEAM_MAX_K || c == 2 + 2 * BEAM_MAX_K) v = -1;   // parent and last token of the root
  if (c == 2 + 6 * BEAM_MAX_K) v = __builtin_bit_cast(int, -__builtin_inff());   // pnb
  state[STATE_HEAD + (long long)b * STATE_SEQ + c] = v;
}

__global__ __launch_bounds__(320) void ctc_beam_chunk_kernel(int* state, const int* __restrict__ n_frames_p, int blank,
                                                              int* hyp, int ld_hyp, int* hyp_len, float* score, int B,
                                                              int T_cap, int chunk_cap, int T_chunk, int K) {
  __shared__ BeamLds L;
  const int b = blockIdx.x, c = threadIdx.x;
  int* H = hyp ? hyp + (long long)b * K * ld_hyp : nullptr;
  const bool geometry = state[0] == STATE_MAGIC && state[1] == B && state[2] == T_cap && state[3] == chunk_cap && state[4] == K;
  int* seq = state + STATE_HEAD + (long long)b * STATE_SEQ;
  const int consumed = geometry ? seq[0] : -1, n = n_frames_p[b];
  if (consumed < 0 || n < 0 || n > T_chunk || (long long)consumed + n > T_cap) {   // workgroup-uniform
    __syncthreads();                      // every thread has read seq[0]
    if (geometry && c == 0) seq[0] = -1;  // dead from here on
    if (H) beam_fail_rows(H, ld_hyp, hyp_len, score, b, K);
    return;
  }
  int* trie_par = state + STATE_HEAD + (long long)B * STATE_SEQ + (long long)b * T_cap * K;
  int* trie_tok = trie_par + (long long)B * T_cap * K;
  const int* top_id = state + STATE_HEAD + (long long)B * STATE_SEQ + 2ll * B * T_cap * K + (long long)b * chunk_cap * K;
  const float* top_lp = (const float*)(top_id + (long long)B * chunk_cap * K);
  const int in = consumed & 1, fin = (consumed + n) & 1;
  beam_clear(L);
  if (c < BEAM_MAX_K) {
    const int* e = seq + 2 + c;
    L.node[in][c] = e[0], L.par[in][c] = e[BEAM_MAX_K], L.last[in][c] = e[2 * BEAM_MAX_K], L.len[in][c] = e[3 * BEAM_MAX_K];
    L.hash[in][c] = (unsigned)e[4 * BEAM_MAX_K];
    L.pb[in][c] = __builtin_bit_cast(float, e[5 * BEAM_MAX_K]), L.pnb[in][c] = __builtin_bit_cast(float, e[6 * BEAM_MAX_K]);
  }
  if (c == 0) L.nb[in] = min(max(seq[1], 0), K);
  __syncthreads();
  beam_frames(L, top_id, top_lp, trie_par, trie_tok, consumed, n, blank, K);
  if (n > 0) {
    if (c < BEAM_MAX_K) {
      int* e = seq + 2 + c;
      e[0] = L.node[fin][c], e[BEAM_MAX_K] = L.par[fin][c], e[2 * BEAM_MAX_K] = L.last[fin][c], e[3 * BEAM_MAX_K] = L.len[fin][c];
      e[4 * BEAM_MAX_K] = (int)L.hash[fin][c];
      e[5 * BEAM_MAX_K] = __builtin_bit_cast(int, L.pb[fin][c]), e[6 * BEAM_MAX_K] = __builtin_bit_cast(int, L.pnb[fin][c]);
    }
    if (c == 0) seq[0] = consumed + n, seq[1] = L.nb[fin];
  }
  if (H) beam_backtrace(L, fin, trie_par, trie_tok, H, ld_hyp, hyp_len, score, b, K);
}

// one wave per row: logits[r][target[r]] - logsumexp(logits[r][:V])
__global__ __launch_bounds__(256) void token_logp_kernel(const float* __restrict__ logits, long long ld,
                                                          const int* __restrict__ target, float* __restrict__ out,
                                                          long long rows, int V) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;   // wave-uniform
  const int tg = target[r];
  if (tg < 0 || tg >= V) {
    if (lane == 0) out[r] = tg < 0 ? 0.f : __builtin_nanf("");
    return;
  }
  const float* row = logits + r * ld;
  float m;
  const float sum = wave_row_sum_exp(row, V, m);
  if (lane == 0) out[r] = (row[tg] - m) - logf(sum);
}

// one wave per row: out[r][v] = x[r][v] - logsumexp(x[r][:V]); out may be x
__global__ __launch_bounds__(256) void log_softmax_rows_kernel(const float* x, long long ldx, float* out, long long ldo,
                                                                long long rows, int V) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;   // wave-uniform
  const float* row = x + r * ldx;
  float m;
  const float lse = logf(wave_row_sum_exp(row, V, m));
  for (int v = lane; v < V; v += 64) out[r * ldo + v] = (row[v] - m) - lse;   // a lane rewrites only what it alone read
}

unsigned long long beam_bytes(int B, int T, int K) { return (unsigned long long)B * T * K * 16ull; }

}  // namespace

int f5e_ctc_beam_workspace_bytes(int B, int T, int beam, unsigned long long* bytes_out_host) {
  F5E_REQUIRE(bytes_out_host, "ctc_beam_workspace_bytes: null output");
  F5E_REQUIRE(B > 0 && T > 0 && T <= BEAM_MAX_T && beam >= 1 && beam <= BEAM_MAX_K,
              "ctc_beam_workspace_bytes: need B > 0, 0 < T <= %d and 1 <= beam <= %d", BEAM_MAX_T, BEAM_MAX_K);
  // per frame and beam slot: the first prune's (class, log p) and the trie's (parent, token)
  *bytes_out_host = beam_bytes(B, T, beam);
  return F5E_OK;
}

int f5e_ctc_beam(hipStream_t st, const float* scores, long long batch_stride, int ld, const int* t_len, int blank, int beam,
                 int* hyp, int ld_hyp, int* hyp_len, float* score, void* workspace, unsigned long long workspace_bytes, int B,
                 int T, int V) {
  F5E_REQUIRE(scores && t_len && hyp && hyp_len && score && workspace, "ctc_beam: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && T <= BEAM_MAX_T, "ctc_beam: need 0 < B <= 65535 and 0 < T <= %d", BEAM_MAX_T);
  F5E_REQUIRE(V >= 2 && blank >= 0 && blank < V, "ctc_beam: need V >= 2 and 0 <= blank < V");
  F5E_REQUIRE(beam >= 1 && beam <= BEAM_MAX_K && beam <= V, "ctc_beam: need 1 <= beam <= %d and beam <= V", BEAM_MAX_K);
  F5E_REQUIRE(ld >= V && ld_hyp >= 1 && (B == 1 || batch_stride >= (long long)(T - 1) * ld + V),
              "ctc_beam: ld / ld_hyp / batch_stride too small");
  F5E_REQUIRE(workspace_bytes >= beam_bytes(B, T, beam) && ((uintptr_t)workspace & 7) == 0,
              "ctc_beam: workspace smaller than f5e_ctc_beam_workspace_bytes or not 8-byte aligned");
  const long long n = (long long)B * T * beam;
  int* top_id = (int*)workspace;
  float* top_lp = (float*)workspace + n;
  int* trie_par = (int*)workspace + 2 * n;
  int* trie_tok = (int*)workspace + 3 * n;
  hipLaunchKernelGGL(ctc_beam_topk_kernel, dim3((unsigned)((T + 3) / 4), (unsigned)B), dim3(256), 0, st, scores, batch_stride,
                     ld, t_len, top_id, top_lp, T, T, V, beam);
  const int threads = (beam + beam * beam + 63) / 64 * 64;
  hipLaunchKernelGGL(ctc_beam_search_kernel, dim3((unsigned)B), dim3((unsigned)threads), 0, st, top_id, top_lp, trie_par,
                     trie_tok, t_len, blank, hyp, ld_hyp, hyp_len, score, T, beam);
  F5E_LAUNCH_CHECK("ctc_beam");
  return F5E_OK;
}

#define BEAM_STATE_GEOMETRY(name)                                                                                          \
  F5E_REQUIRE(B > 0 && B <= 65535 && T_cap > 0 && T_cap <= STATE_MAX_T && chunk_cap > 0 && chunk_cap <= BEAM_MAX_T &&      \
                  beam >= 1 && beam <= BEAM_MAX_K,                                                                         \
              name ": need 0 < B <= 65535, 0 < T_cap <= %d, 0 < chunk_cap <= %d and 1 <= beam <= %d", STATE_MAX_T,         \
              BEAM_MAX_T, BEAM_MAX_K)

int f5e_ctc_beam_state_bytes(int B, int T_cap, int chunk_cap, int beam, unsigned long long* bytes_out_host) {
  F5E_REQUIRE(bytes_out_host, "ctc_beam_state_bytes: null output");
  BEAM_STATE_GEOMETRY("ctc_beam_state_bytes");
  *bytes_out_host = 4ull * state_words(B, T_cap, chunk_cap, beam);
  return F5E_OK;
}

int f5e_ctc_beam_state_init(hipStream_t st, void* state, unsigned long long state_bytes, int B, int T_cap, int chunk_cap,
                            int beam) {
  F5E_REQUIRE(state && ((uintptr_t)state & 7) == 0, "ctc_beam_state_init: state null or not 8-byte aligned");
  BEAM_STATE_GEOMETRY("ctc_beam_state_init");
  F5E_REQUIRE(state_bytes >= 4ull * state_words(B, T_cap, chunk_cap, beam),
              "ctc_beam_state_init: state smaller than f5e_ctc_beam_state_bytes");
  hipLaunchKernelGGL(ctc_beam_state_init_kernel, dim3((unsigned)B), dim3(STATE_SEQ), 0, st, (int*)state, B, T_cap, chunk_cap,
                     beam);
  F5E_LAUNCH_CHECK("ctc_beam_state_init");
  return F5E_OK;
}

int f5e_ctc_beam_chunk(hipStream_t st, const float* scores, long long batch_stride, int ld, const int* n_frames, int T_chunk,
                       int V, int blank, int beam, void* state, unsigned long long state_bytes, int* hyp, int ld_hyp,
                       int* hyp_len, float* score, int B, int T_cap, int chunk_cap) {
  F5E_REQUIRE(scores && n_frames && state, "ctc_beam_chunk: null operand");
  F5E_REQUIRE((hyp && hyp_len && score) || (!hyp && !hyp_len && !score),
              "ctc_beam_chunk: hyp, hyp_len and score are all given or all null");
  BEAM_STATE_GEOMETRY("ctc_beam_chunk");
  F5E_REQUIRE(T_chunk > 0 && T_chunk <= chunk_cap, "ctc_beam_chunk: need 0 < T_chunk <= chunk_cap");
  F5E_REQUIRE(V >= 2 && blank >= 0 && blank < V && beam <= V, "ctc_beam_chunk: need V >= 2, 0 <= blank < V and beam <= V");
  F5E_REQUIRE(ld >= V && (!hyp || ld_hyp >= 1) && (B == 1 || batch_stride >= (long long)(T_chunk - 1) * ld + V),
              "ctc_beam_chunk: ld / ld_hyp / batch_stride too small");
  F5E_REQUIRE(state_bytes >= 4ull * state_words(B, T_cap, chunk_cap, beam) && ((uintptr_t)state & 7) == 0,
              "ctc_beam_chunk: state smaller than f5e_ctc_beam_state_bytes or not 8-byte aligned");
  int* words = (int*)state;
  int* top_id = words + STATE_HEAD + (long long)B * STATE_SEQ + 2ll * B * T_cap * beam;
  float* top_lp = (float*)(top_id + (long long)B * chunk_cap * beam);
  hipLaunchKernelGGL(ctc_beam_topk_kernel, dim3((unsigned)((T_chunk + 3) / 4), (unsigned)B), dim3(256), 0, st, scores,
                     batch_stride, ld, n_frames, top_id, top_lp, T_chunk, chunk_cap, V, beam);
  const int threads = (beam + beam * beam + 63) / 64 * 64;
  hipLaunchKernelGGL(ctc_beam_chunk_kernel, dim3((unsigned)B), dim3((unsigned)threads), 0, st, words, n_frames, blank, hyp,
                     ld_hyp, hyp_len, score, B, T_cap, chunk_cap, T_chunk, beam);
  F5E_LAUNCH_CHECK("ctc_beam_chunk");
  return F5E_OK;
}

int f5e_token_logp(hipStream_t st, const float* logits, long long ld, const int* target, float* out, long long rows, int V) {
  F5E_REQUIRE(logits && target && out, "token_logp: null operand");
  F5E_REQUIRE(rows > 0 && rows <= (1ll << 31) && V >= 1 && ld >= V, "token_logp: need 0 < rows <= 2^31, V >= 1 and ld >= V");
  hipLaunchKernelGGL(token_logp_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, logits, ld, target, out, rows, V);
  F5E_LAUNCH_CHECK("token_logp");
  return F5E_OK;
}

int f5e_log_softmax_rows(hipStream_t st, const float* x, long long ldx, float* out, long long ldo, long long rows, int V) {
  F5E_REQUIRE(x && out, "log_softmax_rows: null operand");
  F5E_REQUIRE(rows > 0 && rows <= (1ll << 31) && V >= 1 && ldx >= V && ldo >= V,
              "log_softmax_rows: need 0 < rows <= 2^31, V >= 1 and ldx, ldo >= V");
  hipLaunchKernelGGL(log_softmax_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, x, ldx, out, ldo, rows, V);
  F5E_LAUNCH_CHECK("log_softmax_rows");
  return F5E_OK;
}
