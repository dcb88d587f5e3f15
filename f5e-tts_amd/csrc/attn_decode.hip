// Autoregressive beam search over the attention decoder (reference ASRModel.recognize, ppg/asr_model.py:309-414): the two
// kernels a decode step needs besides the GEMMs, LayerNorms and f5e_mha_f32 it shares with the full decoder.
//
// ---- f5e_attn_decode_f32: the self-attention of ONE new position p per row against that row's cached keys / values.
// One wave per (row, head).  The step's q | k | v row comes from the fused projection; the wave first files k and v in cache
// slot [r][p] (the only bytes of the caches a launch writes, and nobody reads that slot before the next launch), then
//   1. scores: lane l takes keys l, l + 64, ...: the whole dk-long dot product in registers (q is held by every lane, the key
//      row is read 16 bytes at a time), scaled, into LDS; wave max;
//   2. weights: exp(s - max) back into LDS, wave sum;
//   3. context: lanes split as (key group, channel): consecutive lanes read consecutive channels of one value row; the
//      64 / dk key groups are folded with xor shuffles; channel lanes of group 0 divide by the sum and store.
// Position j < p is read from cache row anc[r][j] (the row in which the hypothesis' ancestor stood when it fed position j) or
// from row r itself when anc is null; position p comes from the registers.  A search therefore never moves cache rows when the
// second prune reshuffles the beam: following the table gives the corrected search (every layer sees its real ancestors),
// passing null reproduces the reference, whose per-layer caches stay with the row index.
// FROM (f5e_attn_decode_from_f32): a row left-padded by begin[r] positions reads positions begin[r] .. p only; the other
// instantiation is the code as it was (lo is the constant 0).
// The K/V read is the traffic: (p + 1) * 2 * dk floats per wave, straight to registers (cdna_hip_programming App. B,
// "attention decode").
//
// ---- f5e_beam_step: asr_model.py:374-403 for all utterances, one workgroup per utterance, one wave per beam row.
//   1. wave w normalises row w (max-subtracted fp32 log-softmax, the form of f5e_log_softmax_rows) and takes its top `beam`
//      classes by `beam` rounds of wave argmax in the order (value descending, class ascending) -- the first prune.  A
//      finished row (its last token is eos, p > 0) contributes (score + 0, eos) and beam - 1 candidates at -inf instead
//      (mask_finished_scores / mask_finished_preds).  Candidate (w, k) = score[w] + logp, in LDS;
//   2. the second prune ranks the beam^2 candidates by counting (value descending, then (parent row, rank) ascending): a
//      candidate's rank is the number of candidates that beat it; ranks < beam are the next beam, in that order;
//   3. the whole workgroup copies the parents' hypothesis / ancestry prefixes into the OTHER table pair (the gather crosses
//      rows) and appends the class at column p + 1, the parent's row at column p.
// No atomics on memory, no sort.
#include "f5e_common.h"
#include "attn_decode_body.h"

namespace {

constexpr int STEP_MAX_K = 16;

// the body (and DEC_MAX_U) is attn_decode_body.h's, shared with the device-position kernel of whisper_step.hip
template <int DK, bool FROM>
__global__ __launch_bounds__(64) void attn_decode_kernel(const float* __restrict__ qkv, int ld_qkv, float* kc, float* vc,
                                                          long long row_stride, int pos_stride, const int* __restrict__ anc,
                                                          int ld_anc, float* __restrict__ out, int ldo, int R, int H, int p,
                                                          float scale, const int* __restrict__ begin) {
  attn_decode_body<DK, FROM>(qkv, ld_qkv, kc, vc, row_stride, pos_stride, anc, ld_anc, out, ldo, R, H, p, scale, begin);
}

__global__ __launch_bounds__(1024) void beam_step_kernel(const float* __restrict__ logits, long long ld_logits, float* score,
                                                          const int* __restrict__ hyp_in, const int* __restrict__ anc_in,
                                                          int* __restrict__ hyp_out, int* __restrict__ anc_out, int ld,
                                                          int* __restrict__ last, int* __restrict__ alive,
                                                          int* __restrict__ done_at, int p, int K, int eos, int V) {
  __shared__ unsigned c_key[STEP_MAX_K * STEP_MAX_K];
  __shared__ float c_val[STEP_MAX_K * STEP_MAX_K];
  __shared__ int c_cls[STEP_MAX_K * STEP_MAX_K];
  __shared__ int sel_par[STEP_MAX_K], sel_cls[STEP_MAX_K];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;   // blockDim.x = 64 K: wave w = beam row w
  const long long r0 = (long long)b * K, r = r0 + w;
  const float NEG = -__builtin_inff();

  // ---- 1. first prune of row r
  {
    const float sc = score[r];
    const bool finished = p > 0 && hyp_in[r * ld + p] == eos;   // wave-uniform
    if (finished) {
      if (lane < K) {
        const float v = lane == 0 ? sc : NEG;
        c_val[w * K + lane] = v, c_key[w * K + lane] = rank_key(v), c_cls[w * K + lane] = eos;
      }
    } else {
      const float* row = logits + r * ld_logits;
      float pv = __builtin_inff(), m0 = 0.f, lse = 0.f;
      int pi = -1;
      for (int k = 0; k < K; ++k) {
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
        if (k == 0) {
          float sum = 0.f;
          for (int v = lane; v < V; v += 64) sum += expf(row[v] - m);
          lse = logf(wave_sum(sum));
          m0 = m;
        }
        if (lane == 0) {
          const bool none = arg == 0x7fffffff;   // fewer than K comparable values (NaN in the row)
          const float v = none ? NEG : sc + ((m - m0) - lse);
          c_val[w * K + k] = v, c_key[w * K + k] = rank_key(v), c_cls[w * K + k] = none ? eos : arg;
        }
        pv = m, pi = arg;
      }
    }
  }
  __syncthreads();
  // ---- 2. second prune: rank by counting
  const int NC = K * K;
  if (tid < NC) {
    const unsigned k = c_key[tid];
    int rank = 0;
    for (int i = 0; i < NC; ++i) {
      const unsigned o = c_key[i];
      rank += o > k || (o == k && i < tid);
    }
    if (rank < K) {
      sel_par[rank] = tid / K, sel_cls[rank] = c_cls[tid];
      score[r0 + rank] = c_val[tid];   // every old score was read before the barrier
      last[r0 + rank] = c_cls[tid];
    }
  }
  __syncthreads();
  // ---- 3. gather the parents' prefixes, append
  const int n_h = p + 2, n_a = p + 1;   // hypothesis columns 0..p+1, ancestry columns 0..p
  for (int i = tid; i < K * n_h; i += blockDim.x) {
    const int q = i / n_h, c = i % n_h;
    hyp_out[(r0 + q) * ld + c] = c == p + 1 ? sel_cls[q] : hyp_in[(r0 + sel_par[q]) * ld + c];
  }
  for (int i = tid; i < K * n_a; i += blockDim.x) {
    const int q = i / n_a, c = i % n_a;
    anc_out[(r0 + q) * ld + c] = c == p ? (int)r0 + sel_par[q] : anc_in[(r0 + sel_par[q]) * ld + c];
  }
  if (tid == 0) {
    int n = 0;
    for (int q = 0; q < K; ++q) n += sel_cls[q] != eos;
    alive[b] = n;
    if (n == 0 && done_at[b] < 0) done_at[b] = p;
  }
}

}  // namespace

static int attn_decode_launch(hipStream_t st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                              int pos_stride, const int* anc, int ld_anc, const int* begin, float* out, int ldo, int R, int Umax,
                              int H, int dk, int p, float scale) {
  F5E_REQUIRE(qkv && kc && vc && out, "attn_decode_f32: null operand");
  F5E_REQUIRE(R > 0 && R <= 65535 && H > 0 && H <= 65535, "attn_decode_f32: need 0 < R, H <= 65535");
  F5E_REQUIRE(dk == 16 || dk == 32 || dk == 64 || dk == 128, "attn_decode_f32: head dim must be 16, 32, 64 or 128");
  F5E_REQUIRE(Umax > 0 && Umax <= DEC_MAX_U && p >= 0 && p < Umax, "attn_decode_f32: need 0 <= p < Umax <= %d", DEC_MAX_U);
  const long long HD = (long long)H * dk;
  F5E_REQUIRE(ld_qkv >= 3 * HD && ldo >= HD && pos_stride >= HD && row_stride >= (long long)(Umax - 1) * pos_stride + HD,
              "attn_decode_f32: a stride is smaller than the data it spans");
  F5E_REQUIRE(ld_qkv % 4 == 0 && pos_stride % 4 == 0 && row_stride % 4 == 0 && ((uintptr_t)qkv & 15) == 0 &&
                  ((uintptr_t)kc & 15) == 0,
              "attn_decode_f32: qkv / cache strides must be multiples of 4 floats, qkv and kc 16-byte aligned");
  F5E_REQUIRE(!anc || ld_anc >= p, "attn_decode_f32: the ancestry table has fewer than p columns");
  const dim3 grid((unsigned)H, (unsigned)R), block(64);
#define F5E_DEC_LAUNCH(DK)                                                                                                   \
  if (begin)                                                                                                                 \
    hipLaunchKernelGGL((attn_decode_kernel<DK, true>), grid, block, 0, st, qkv, ld_qkv, kc, vc, row_stride, pos_stride, anc, \
                       ld_anc, out, ldo, R, H, p, scale, begin);                                                             \
  else                                                                                                                       \
    hipLaunchKernelGGL((attn_decode_kernel<DK, false>), grid, block, 0, st, qkv, ld_qkv, kc, vc, row_stride, pos_stride,     \
                       anc, ld_anc, out, ldo, R, H, p, scale, begin)
  switch (dk) {
    case 16: F5E_DEC_LAUNCH(16); break;
    case 32: F5E_DEC_LAUNCH(32); break;
    case 64: F5E_DEC_LAUNCH(64); break;
    default: F5E_DEC_LAUNCH(128); break;
  }
#undef F5E_DEC_LAUNCH
  F5E_LAUNCH_CHECK("attn_decode_f32");
  return F5E_OK;
}

int f5e_attn_decode_f32(hipStream_t st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                        int pos_stride, const int* anc, int ld_anc, float* out, int ldo, int R, int Umax, int H, int dk, int p,
                        float scale) {
  return attn_decode_launch(st, qkv, ld_qkv, kc, vc, row_stride, pos_stride, anc, ld_anc, nullptr, out, ldo, R, Umax, H, dk, p,
                            scale);
}

int f5e_attn_decode_from_f32(hipStream_t st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                             int pos_stride, const int* anc, int ld_anc, const int* begin, float* out, int ldo, int R, int Umax,
                             int H, int dk, int p, float scale) {
  return attn_decode_launch(st, qkv, ld_qkv, kc, vc, row_stride, pos_stride, anc, ld_anc, begin, out, ldo, R, Umax, H, dk, p,
                            scale);
}

int f5e_beam_step(hipStream_t st, const float* logits, long long ld_logits, float* score, const int* hyp_in, const int* anc_in,
                  int* hyp_out, int* anc_out, int ld, int* last, int* alive, int* done_at, int B, int V, int beam, int p,
                  int eos) {
  F5E_REQUIRE(logits && score && hyp_in && anc_in && hyp_out && anc_out && last && alive && done_at,
              "beam_step: null operand");
  F5E_REQUIRE(hyp_in != hyp_out && anc_in != anc_out, "beam_step: the hyp / anc tables are double-buffered (in != out)");
  F5E_REQUIRE(B > 0 && B <= 65535 && V >= 1 && ld_logits >= V, "beam_step: need 0 < B <= 65535, V >= 1 and ld_logits >= V");
  F5E_REQUIRE(beam >= 1 && beam <= STEP_MAX_K && beam <= V, "beam_step: need 1 <= beam <= %d and beam <= V", STEP_MAX_K);
  F5E_REQUIRE(p >= 0 && ld >= p + 2, "beam_step: need p >= 0 and tables of at least p + 2 columns");
  F5E_REQUIRE(eos >= 0 && eos < V, "beam_step: need 0 <= eos < V");
  hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)B), dim3((unsigned)(64 * beam)), 0, st, logits, ld_logits, score, hyp_in,
                     anc_in, hyp_out, anc_out, ld, last, alive, done_at, p, beam, eos, V);
  F5E_LAUNCH_CHECK("beam_step");
  return F5E_OK;
}
