// CTC prefix beam search on the device (f5e_ctc_beam), the per-row target log-probability of the rescoring sum
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

__device__ __forceinline__ float logaddexp_f(float a, float b) {
  const float m = fmaxf(a, b), n = fminf(a, b);
  if (!(m > -__builtin_inff())) return m;   // both -inf
  return m + log1pf(expf(n - m));
}

// order-preserving float -> unsigned key, never 0 (0 = "no candidate"); NaN ranks as -inf
__device__ __forceinline__ unsigned rank_key(float v) {
  if (v != v) v = -__builtin_inff();
  const unsigned u = __builtin_bit_cast(unsigned, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned hash_step(unsigned h, int tok) {
  h ^= (unsigned)tok + 0x9e3779b9u + (h << 6) + (h >> 2);
  return h * 0x85ebca6bu;
}

// one wave per frame: top K classes (value descending, class ascending) and their log-probabilities
__global__ __launch_bounds__(256) void ctc_beam_topk_kernel(const float* __restrict__ scores, long long batch_stride, int ld,
                                                             const int* __restrict__ t_len_p, int* __restrict__ top_id,
                                                             float* __restrict__ top_lp, int T, int V, int K) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  const int t_len = t_len_p[b];
  if (t >= T || t_len > T || t >= t_len) return;   // wave-uniform
  const float* row = scores + (long long)b * batch_stride + (long long)t * ld;
  const float NEG = -__builtin_inff();
  float pv = __builtin_inff(), m0 = 0.f, lse = 0.f;
  int pi = -1;
  for (int r = 0; r < K; ++r) {
    float m = NEG;
    int arg = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
      const float x = row[v];
      const bool after = x < pv || (x == pv && v > pi);
      if (after && (arg == 0x7fffffff || x > m)) m = x, arg = v;   // ascending v per lane: the first maximum stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oa = __shfl_xor(arg, o, 64);
      if (om > m || (om == m && oa < arg)) m = om, arg = oa;
    }
    if (r == 0) {
      float sum = 0.f;
      for (int v = lane; v < V; v += 64) sum += v == arg ? 0.f : expf(row[v] - m);
      lse = log1pf(wave_sum(sum));
      m0 = m;
    }
    if (lane == 0) {
      const long long o = ((long long)b * T + t) * K + r;
      const bool none = arg == 0x7fffffff;   // fewer than K comparable values (NaN in the row)
      top_id[o] = none ? -1 : arg;
      top_lp[o] = none ? NEG : (m - m0) - lse;
    }
    pv = m, pi = arg;
  }
}

__global__ __launch_bounds__(320) void ctc_beam_search_kernel(const int* __restrict__ top_id, const float* __restrict__ top_lp,
                                                               int* trie_par, int* trie_tok,
                                                               const int* __restrict__ t_len_p, int blank,
                                                               int* __restrict__ hyp, int ld_hyp, int* __restrict__ hyp_len,
                                                               float* __restrict__ score, int T, int K) {
  __shared__ int b_node[2][BEAM_MAX_K], b_par[2][BEAM_MAX_K], b_last[2][BEAM_MAX_K], b_len[2][BEAM_MAX_K];
  __shared__ unsigned b_hash[2][BEAM_MAX_K];
  __shared__ float b_pb[2][BEAM_MAX_K], b_pnb[2][BEAM_MAX_K];
  __shared__ int nb_s[2];
  __shared__ float s_blank[BEAM_MAX_K], s_rep[BEAM_MAX_K], s_merge[BEAM_MAX_K];
  __shared__ int f_blank[BEAM_MAX_K], f_rep[BEAM_MAX_K], f_merge[BEAM_MAX_K];
  __shared__ __attribute__((aligned(16))) unsigned key[BEAM_MAX_C];
  const int b = blockIdx.x, c = threadIdx.x, nt = blockDim.x;
  const int NC = K + K * K, NC4 = (NC + 3) & ~3;
  const float NEG = -__builtin_inff();
  const int t_len = t_len_p[b];
  int* H = hyp + (long long)b * K * ld_hyp;
  if (t_len < 0 || t_len > T) {   // workgroup-uniform: -1 / -inf rows, defined and harmless
    for (long long i = c; i < (long long)K * ld_hyp; i += nt) H[i] = -1;
    if (c < K) hyp_len[(long long)b * K + c] = -1, score[(long long)b * K + c] = NEG;
    return;
  }
  const long long base = (long long)b * T * K;
  top_id += base, top_lp += base, trie_par += base, trie_tok += base;

  if (c < BEAM_MAX_K) f_blank[c] = f_rep[c] = f_merge[c] = 0;
  for (int i = c; i < BEAM_MAX_C; i += nt) key[i] = 0;
  if (c == 0) {   // the empty prefix: the trie's root, node 0
    b_node[0][0] = 0, b_par[0][0] = -1, b_last[0][0] = -1, b_len[0][0] = 0, b_hash[0][0] = 0;
    b_pb[0][0] = 0.f, b_pnb[0][0] = NEG;
    nb_s[0] = 1;
  }
  const bool is_stay = c < K, is_cell = c >= K && c < NC;
  const int p = is_cell ? (c - K) / K : c, j = is_cell ? (c - K) % K : 0;
  int s = -1;
  float ps = NEG;
  if (is_cell && t_len > 0) s = top_id[j], ps = top_lp[j];
  __syncthreads();

  for (int t = 0; t < t_len; ++t) {
    const int cur = t & 1, nxt = cur ^ 1;
    const int nb = nb_s[cur];
    // ---- 1. the cells
    float val = NEG, n_pb = NEG, n_pnb = NEG;
    int node_p = 0, len_p = 0;
    unsigned hash_n = 0, k = 0;
    if (c == 0) nb_s[nxt] = 0;
    if (is_cell && p < nb && s >= 0) {
      node_p = b_node[cur][p], len_p = b_len[cur][p];
      const int last_p = b_last[cur][p];
      const float pb = b_pb[cur][p], pnb = b_pnb[cur][p];
      const float both = logaddexp_f(pb + ps, pnb + ps);
      if (s == blank) {
        s_blank[p] = both, f_blank[p] = 1;
      } else {
        if (s == last_p) s_rep[p] = pnb + ps, f_rep[p] = 1;
        val = s == last_p ? pb + ps : both;
        hash_n = hash_step(b_hash[cur][p], s);
        int q = -1;
        for (int i = 0; i < nb; ++i) {
          if (b_last[cur][i] != s || b_len[cur][i] != len_p + 1) continue;
          int x = b_par[cur][i], y = node_p;
          if (x != y && b_hash[cur][i] != hash_n) continue;
          bool same = true;   // both chains hold len_p tokens: they meet at a common node (the root at the latest) or differ
          while (x != y) {
            if (x <= 0 || y <= 0 || trie_tok[x - 1] != trie_tok[y - 1]) {
              same = false;
              break;
            }
            x = trie_par[x - 1], y = trie_par[y - 1];
          }
          if (same) q = i;
        }
        if (q >= 0) s_merge[q] = val, f_merge[q] = 1;   // one writer: q's prefix minus its last token is one beam entry
        else k = rank_key(val);
      }
    }
    if (is_cell) key[c] = k;
    int s_next = -1;
    float ps_next = NEG;
    if (is_cell && t + 1 < t_len) s_next = top_id[(t + 1) * K + j], ps_next = top_lp[(t + 1) * K + j];
    __syncthreads();
    // ---- 2. the stay candidates
    if (is_stay) {
      k = 0;
      if (c < nb && (f_blank[c] | f_rep[c] | f_merge[c])) {
        n_pb = f_blank[c] ? s_blank[c] : NEG;
        n_pnb = logaddexp_f(f_rep[c] ? s_rep[c] : NEG, f_merge[c] ? s_merge[c] : NEG);
        k = rank_key(logaddexp_f(n_pb, n_pnb));
      }
      key[c] = k;
    }
    __syncthreads();
    // ---- 3. rank by counting; ranks < K are the next beam
    if (c < BEAM_MAX_K) f_blank[c] = f_rep[c] = f_merge[c] = 0;
    if (k != 0) {
      int rank = 0;
      for (int i = 0; i < NC4; i += 4) {
        const uint4 o = *(const uint4*)&key[i];
        rank += (o.x > k || (o.x == k && i < c)) + (o.y > k || (o.y == k && i + 1 < c)) +
                (o.z > k || (o.z == k && i + 2 < c)) + (o.w > k || (o.w == k && i + 3 < c));
      }
      if (rank < K) {
        atomicAdd(&nb_s[nxt], 1);
        if (is_stay) {
          b_node[nxt][rank] = b_node[cur][c], b_par[nxt][rank] = b_par[cur][c], b_last[nxt][rank] = b_last[cur][c];
          b_len[nxt][rank] = b_len[cur][c], b_hash[nxt][rank] = b_hash[cur][c];
          b_pb[nxt][rank] = n_pb, b_pnb[nxt][rank] = n_pnb;
        } else {
          const int slot = t * K + rank;   // < T K: inside the sequence's share of the workspace
          b_node[nxt][rank] = 1 + slot, b_par[nxt][rank] = node_p, b_last[nxt][rank] = s;
          b_len[nxt][rank] = len_p + 1, b_hash[nxt][rank] = hash_n;
          b_pb[nxt][rank] = NEG, b_pnb[nxt][rank] = val;
          trie_par[slot] = node_p, trie_tok[slot] = s;
        }
      }
    }
    s = s_next, ps = ps_next;
    // the trie is read back by other threads of this workgroup: a workgroup-scope release, then the barrier
    __threadfence_block();
    __syncthreads();
  }

  // ---- backtrace: lane q walks hypothesis q; the -1 padding is dealt over the whole workgroup
  const int fin = t_len & 1, nb = min(nb_s[fin], K);
  for (int q = 0; q < K; ++q) {
    const int from = q < nb ? min(b_len[fin][q], ld_hyp) : 0;
    for (int i = from + c; i < ld_hyp; i += nt) H[(long long)q * ld_hyp + i] = -1;
  }
  if (c < K) {
    int len = -1;
    float sc = NEG;
    if (c < nb) {
      len = b_len[fin][c];
      sc = logaddexp_f(b_pb[fin][c], b_pnb[fin][c]);
      int node = b_node[fin][c];
      for (int pos = len - 1; pos >= 0 && node > 0; --pos) {
        if (pos < ld_hyp) H[(long long)c * ld_hyp + pos] = trie_tok[node - 1];
        node = trie_par[node - 1];
      }
    }
    hyp_len[(long long)b * K + c] = len;
    score[(long long)b * K + c] = sc;
  }
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
  float m = -__builtin_inff();
  for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
  m = wave_max(m);
  float sum = 0.f;
  for (int v = lane; v < V; v += 64) sum += expf(row[v] - m);
  sum = wave_sum(sum);
  if (lane == 0) out[r] = (row[tg] - m) - logf(sum);
}

// one wave per row: out[r][v] = x[r][v] - logsumexp(x[r][:V]); out may be x
__global__ __launch_bounds__(256) void log_softmax_rows_kernel(const float* x, long long ldx, float* out, long long ldo,
                                                                long long rows, int V) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;   // wave-uniform
  const float* row = x + r * ldx;
  float m = -__builtin_inff();
  for (int v = lane; v < V; v += 64) m = fmaxf(m, row[v]);
  m = wave_max(m);
  float sum = 0.f;
  for (int v = lane; v < V; v += 64) sum += expf(row[v] - m);
  const float lse = logf(wave_sum(sum));
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
                     ld, t_len, top_id, top_lp, T, V, beam);
  const int threads = (beam + beam * beam + 63) / 64 * 64;
  hipLaunchKernelGGL(ctc_beam_search_kernel, dim3((unsigned)B), dim3((unsigned)threads), 0, st, top_id, top_lp, trie_par,
                     trie_tok, t_len, blank, hyp, ld_hyp, hyp_len, score, T, beam);
  F5E_LAUNCH_CHECK("ctc_beam");
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
