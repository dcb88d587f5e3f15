// Whisper's cached decode step with the position on the DEVICE, so that one step can be captured into a hipGraph once and
// replayed per token ("the captured step").  Everything that changes from token to token lives in the step record,
// 8 x i32, 16-byte aligned, which the kernels read and one thread advances:
//
//   rec[0] p          the position the step feeds (the pick writes token column p + 1)
//   rec[1] n0         the prompt length: the generated tokens of a row are tokens[r][n0 .. p]; first_step = (p + 1 == n0)
//   rec[2] seed_lo    the sampled pick's Philox key, low and high word of the 64-bit seed
//   rec[3] seed_hi
//   rec[4] temp       the sampled pick's temperature, the bits of an fp32 (> 0, finite; anything else draws at T = 1)
//   rec[5..7]         reserved, never written by a kernel
//
// The bodies are the eager step's own (attn_decode_body.h, whisper_pick.h), so a replayed step gives the eager step's bits.
// Every kernel clamps what it reads from the record to the extents it was launched with (P cached positions, the position
// table's rows, the token table's width): a wrong record can put a result in the wrong slot, never outside a buffer.
// Grids do not depend on the record.  No kernel waits for another workgroup: the stream is the only ordering, and p is
// advanced by thread 0 of the one-workgroup launch that follows the pick (the last reader of the step).
//
//   f5e_attn_decode_dev_f32       attn_decode_kernel with anc == null, with and without begin
//   f5e_whisper_embed_dev         x[r] = emb[last[r]] + pos[max(p - begin[r], 0)]
//   f5e_greedy_pick_dev           f5e_greedy_pick          + advance
//   f5e_whisper_ts_pick_dev       f5e_whisper_ts_pick      + advance
//   f5e_whisper_sample_pick_dev   f5e_whisper_sample_pick  + advance
#include "f5e_common.h"
#include "w_load.h"
#include "attn_decode_body.h"
#include "whisper_pick.h"

namespace {

constexpr int REC_P = 0, REC_N0 = 1, REC_SEED_LO = 2, REC_SEED_HI = 3, REC_TEMP = 4;

// p for a table of `width` columns: the pick writes column p + 1 <= width - 1
__device__ __forceinline__ int rec_pick_p(const int* __restrict__ rec, int width) { return min(max(rec[REC_P], 0), width - 2); }
// n0 in [1, p + 1]: the history tokens[r][n0 .. p] is never longer than the row nor of negative length
__device__ __forceinline__ int rec_pick_n0(const int* __restrict__ rec, int p) { return min(max(rec[REC_N0], 1), p + 1); }

template <int DK, bool FROM>
__global__ __launch_bounds__(64) void attn_decode_dev_kernel(const float* __restrict__ qkv, int ld_qkv, float* kc, float* vc,
                                                              long long row_stride, int pos_stride, float* __restrict__ out,
                                                              int ldo, int R, int H, int P, const int* __restrict__ rec,
                                                              float scale, const int* __restrict__ begin) {
  const int p = min(max(rec[REC_P], 0), P - 1);
  attn_decode_body<DK, FROM>(qkv, ld_qkv, kc, vc, row_stride, pos_stride, nullptr, 0, out, ldo, R, H, p, scale, begin);
}

template <class WL>   // the token table's loader (w_load.h): fp32, or 16-bit widened in registers
__global__ __launch_bounds__(256) void embed_dev_kernel(const int* __restrict__ last, const int* __restrict__ begin,
                                                        const typename WL::elem* __restrict__ emb, const float* __restrict__ pos,
                                                        float* __restrict__ out, int R, int D, const int* __restrict__ rec,
                                                        int max_pos, int table_rows) {
  const int d4 = D / 4, p = rec[REC_P];
  const size_t total = (size_t)R * d4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % d4) * 4, r = (int)(i / d4);
    const int id = min(max(last[r], 0), table_rows - 1);
    const int b = begin ? begin[r] : 0;
    const int at = min(max(p, 0) - min(max(b, 0), max(p, 0)), max_pos - 1);   // max(p - begin[r], 0), without overflow
    *(f32x4*)(out + (size_t)r * D + c) = WL::load4(emb + (size_t)id * D + c) + *(const f32x4*)(pos + (size_t)at * D + c);
  }
}

__global__ __launch_bounds__(256) void greedy_pick_dev_kernel(const float* __restrict__ logits, long long ld,
                                                              const int* __restrict__ suppress, int n_sup,
                                                              const int* __restrict__ begin_suppress, int n_beg, int* tokens,
                                                              int ld_tok, int n_tok, int* last, int* done, int V,
                                                              const int* __restrict__ rec, int eos) {
  const int p = rec_pick_p(rec, n_tok);
  greedy_pick_step(logits, ld, suppress, n_sup, begin_suppress, p + 1 == rec[REC_N0] ? n_beg : 0, tokens, ld_tok, last, done, V, p,
                   eos);
}

__global__ __launch_bounds__(256) void ts_pick_dev_kernel(const float* __restrict__ logits, long long ld,
                                                          const int* __restrict__ suppress, int n_sup,
                                                          const int* __restrict__ begin_suppress, int n_beg, int* tokens,
                                                          int ld_tok, int n_tok, int* last, int* done, float* sum_logp, int V,
                                                          const int* __restrict__ rec, int eos, int no_ts, int max_initial) {
  const int p = rec_pick_p(rec, n_tok), n0 = rec_pick_n0(rec, p);
  ts_rule_step<true>(logits, ld, suppress, n_sup, begin_suppress, p + 1 == n0 ? n_beg : 0, tokens, ld_tok, last, done, sum_logp,
                     nullptr, V, p, n0, eos, no_ts, max_initial);
}

__global__ __launch_bounds__(256) void sample_pick_dev_kernel(const float* __restrict__ logits, long long ld,
                                                              const int* __restrict__ suppress, int n_sup,
                                                              const int* __restrict__ begin_suppress, int n_beg, int* tokens,
                                                              int ld_tok, int n_tok, int* last, int* done, float* sum_logp, int V,
                                                              const int* __restrict__ rec, int eos, int no_ts, int max_initial,
                                                              const int* __restrict__ row_key, const int* __restrict__ serial) {
  const int p = rec_pick_p(rec, n_tok), n0 = rec_pick_n0(rec, p);
  float temperature = __int_as_float(rec[REC_TEMP]);
  if (!(temperature > 0.f && temperature < __builtin_inff())) temperature = 1.f;
  ts_sample_step(logits, ld, suppress, n_sup, begin_suppress, p + 1 == n0 ? n_beg : 0, tokens, ld_tok, last, done, sum_logp, V, p, n0,
                 eos, no_ts, max_initial, temperature, (unsigned)rec[REC_SEED_LO], (unsigned)rec[REC_SEED_HI], row_key, serial);
}

// alive_count_kernel, and the step's one writer of p: this launch is a single workgroup behind the pick, the step's last reader.
__global__ __launch_bounds__(256) void alive_advance_kernel(const int* __restrict__ done, int* __restrict__ alive, int R, int* rec) {
  __shared__ int red[4];
  const int n = alive_count_rows(done, R, red);
  if (threadIdx.x == 0) {
    *alive = n;
    const int p = rec[REC_P];
    rec[REC_P] = p < 0x7ffffffe ? p + 1 : p;
  }
}

int pick_dev_check(const char* name, const float* logits, long long ld, const int* suppress, int n_sup, const int* begin_suppress,
                   int n_beg, const int* tokens, int ld_tok, int n_tok, const int* last, const int* done, const int* alive, const int* rec,
                   int R, int V, int eos, int min_V) {
  F5E_REQUIRE(logits && tokens && last && done && alive && rec, "%s: null operand", name);
  F5E_REQUIRE(((uintptr_t)rec & 15) == 0, "%s: the step record must be 16-byte aligned", name);
  F5E_REQUIRE(R > 0 && R <= 0x7fffffff / 2 && V >= min_V && V <= GP_MAX_V && ld >= V,
              "%s: need R > 0, %d <= V <= %d and ld >= V (R=%d V=%d)", name, min_V, GP_MAX_V, R, V);
  F5E_REQUIRE(n_sup >= 0 && n_beg >= 0 && (n_sup == 0 || suppress) && (n_beg == 0 || begin_suppress),
              "%s: a suppression list without its pointer", name);
  F5E_REQUIRE(n_tok >= 2 && ld_tok >= n_tok, "%s: token rows need 2 <= n_tok <= ld_tok columns (n_tok=%d ld_tok=%d)", name, n_tok,
              ld_tok);
  F5E_REQUIRE(eos >= 0 && eos < V, "%s: need 0 <= eos < V", name);
  return F5E_OK;
}

#define F5E_TS_DEV_REQUIRE(name)                                                                                              \
  F5E_REQUIRE(no_timestamps >= 0 && no_timestamps + 1 < V && eos <= no_timestamps && max_initial >= -1,                        \
              name ": need 0 <= eos <= no_timestamps < V - 1 and max_initial >= -1 (eos=%d no_timestamps=%d V=%d "              \
                   "max_initial=%d)", eos, no_timestamps, V, max_initial)

inline int grid_for(size_t total) {
  size_t g = (total + 255) / 256;
  return (int)(g < 4096 ? (g ? g : 1) : 4096);
}

}  // namespace

extern "C" int f5e_attn_decode_dev_f32(hipStream_t st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                                       int pos_stride, const int* begin, float* out, int ldo, int R, int P, int H, int dk,
                                       const int* rec, float scale) {
  F5E_REQUIRE(qkv && kc && vc && out && rec, "attn_decode_dev_f32: null operand");
  F5E_REQUIRE(R > 0 && R <= 65535 && H > 0 && H <= 65535, "attn_decode_dev_f32: need 0 < R, H <= 65535");
  F5E_REQUIRE(dk == 16 || dk == 32 || dk == 64 || dk == 128, "attn_decode_dev_f32: head dim must be 16, 32, 64 or 128");
  F5E_REQUIRE(P > 0 && P <= DEC_MAX_U, "attn_decode_dev_f32: need 0 < P <= %d cached positions", DEC_MAX_U);
  const long long HD = (long long)H * dk;
  F5E_REQUIRE(ld_qkv >= 3 * HD && ldo >= HD && pos_stride >= HD && row_stride >= (long long)(P - 1) * pos_stride + HD,
              "attn_decode_dev_f32: a stride is smaller than the data it spans");
  F5E_REQUIRE(ld_qkv % 4 == 0 && pos_stride % 4 == 0 && row_stride % 4 == 0 && ((uintptr_t)qkv & 15) == 0 &&
                  ((uintptr_t)kc & 15) == 0 && ((uintptr_t)rec & 15) == 0,
              "attn_decode_dev_f32: qkv / cache strides must be multiples of 4 floats, qkv, kc and the record 16-byte aligned");
  const dim3 grid((unsigned)H, (unsigned)R), block(64);
#define F5E_DEC_DEV_LAUNCH(DK)                                                                                                 \
  if (begin)                                                                                                                   \
    hipLaunchKernelGGL((attn_decode_dev_kernel<DK, true>), grid, block, 0, st, qkv, ld_qkv, kc, vc, row_stride, pos_stride, out, \
                       ldo, R, H, P, rec, scale, begin);                                                                       \
  else                                                                                                                         \
    hipLaunchKernelGGL((attn_decode_dev_kernel<DK, false>), grid, block, 0, st, qkv, ld_qkv, kc, vc, row_stride, pos_stride,    \
                       out, ldo, R, H, P, rec, scale, begin)
  switch (dk) {
    case 16: F5E_DEC_DEV_LAUNCH(16); break;
    case 32: F5E_DEC_DEV_LAUNCH(32); break;
    case 64: F5E_DEC_DEV_LAUNCH(64); break;
    default: F5E_DEC_DEV_LAUNCH(128); break;
  }
#undef F5E_DEC_DEV_LAUNCH
  F5E_LAUNCH_CHECK("attn_decode_dev_f32");
  return F5E_OK;
}

template <class WL>
static int embed_dev_launch(const char* name, hipStream_t st, const int* last, const int* begin, const void* emb, int emb_align,
                            const float* pos, float* out, int R, int D, const int* rec, int max_pos, int table_rows) {
  F5E_REQUIRE(last && emb && pos && out && rec, "%s: null operand", name);
  F5E_REQUIRE(R > 0 && D > 0 && D % 4 == 0 && table_rows > 0 && max_pos > 0,
              "%s: need R > 0, D a multiple of 4 and non-empty tables (R=%d D=%d max_pos=%d)", name, R, D, max_pos);
  F5E_REQUIRE((((uintptr_t)pos | (uintptr_t)out | (uintptr_t)rec) & 15) == 0 && ((uintptr_t)emb & (uintptr_t)(emb_align - 1)) == 0,
              "%s: emb, pos, out and the record must be 16-byte aligned (a 16-bit emb: 8-byte)", name);
  hipLaunchKernelGGL(embed_dev_kernel<WL>, dim3(grid_for((size_t)R * D / 4)), dim3(256), 0, st, last, begin,
                     (const typename WL::elem*)emb, pos, out, R, D, rec, max_pos, table_rows);
  F5E_LAUNCH_CHECK(name);
  return F5E_OK;
}

extern "C" int f5e_whisper_embed_dev(hipStream_t st, const int* last, const int* begin, const float* emb, const float* pos,
                                     float* out, int R, int D, const int* rec, int max_pos, int table_rows) {
  return embed_dev_launch<WLoadF32>("whisper_embed_dev", st, last, begin, emb, 16, pos, out, R, D, rec, max_pos, table_rows);
}

extern "C" int f5e_whisper_embed_w16_dev(hipStream_t st, const int* last, const int* begin, const void* emb, int wtype,
                                         const float* pos, float* out, int R, int D, const int* rec, int max_pos, int table_rows) {
  F5E_REQUIRE(wtype == F5E_W_FP16 || wtype == F5E_W_BF16, "whisper_embed_w16_dev: wtype %d is neither F5E_W_FP16 nor F5E_W_BF16",
              wtype);
  if (wtype == F5E_W_FP16)
    return embed_dev_launch<WLoad16<F5E_W_FP16>>("whisper_embed_w16_dev", st, last, begin, emb, 8, pos, out, R, D, rec, max_pos,
                                                 table_rows);
  return embed_dev_launch<WLoad16<F5E_W_BF16>>("whisper_embed_w16_dev", st, last, begin, emb, 8, pos, out, R, D, rec, max_pos,
                                               table_rows);
}

extern "C" int f5e_greedy_pick_dev(hipStream_t st, const float* logits, long long ld, const int* suppress, int n_sup,
                                   const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int n_tok, int* last, int* done, int* alive,
                                   int R, int V, int* rec, int eos) {
  const int rc = pick_dev_check("greedy_pick_dev", logits, ld, suppress, n_sup, begin_suppress, n_beg, tokens, ld_tok, n_tok, last, done,
                                alive, rec, R, V, eos, 1);
  if (rc != F5E_OK) return rc;
  hipLaunchKernelGGL(greedy_pick_dev_kernel, dim3((unsigned)R), dim3(256), 0, st, logits, ld, suppress, n_sup, begin_suppress,
                     n_beg, tokens, ld_tok, n_tok, last, done, V, rec, eos);
  hipLaunchKernelGGL(alive_advance_kernel, dim3(1), dim3(256), 0, st, done, alive, R, rec);
  F5E_LAUNCH_CHECK("greedy_pick_dev");
  return F5E_OK;
}

extern "C" int f5e_whisper_ts_pick_dev(hipStream_t st, const float* logits, long long ld, const int* suppress, int n_sup,
                                       const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int n_tok, int* last, int* done,
                                       int* alive, float* sum_logp, int R, int V, int* rec, int eos, int no_timestamps,
                                       int max_initial) {
  F5E_REQUIRE(sum_logp, "whisper_ts_pick_dev: null operand");
  const int rc = pick_dev_check("whisper_ts_pick_dev", logits, ld, suppress, n_sup, begin_suppress, n_beg, tokens, ld_tok, n_tok, last,
                                done, alive, rec, R, V, eos, 2);
  if (rc != F5E_OK) return rc;
  F5E_TS_DEV_REQUIRE("whisper_ts_pick_dev");
  hipLaunchKernelGGL(ts_pick_dev_kernel, dim3((unsigned)R), dim3(256), 0, st, logits, ld, suppress, n_sup, begin_suppress, n_beg,
                     tokens, ld_tok, n_tok, last, done, sum_logp, V, rec, eos, no_timestamps, max_initial);
  hipLaunchKernelGGL(alive_advance_kernel, dim3(1), dim3(256), 0, st, done, alive, R, rec);
  F5E_LAUNCH_CHECK("whisper_ts_pick_dev");
  return F5E_OK;
}

extern "C" int f5e_whisper_sample_pick_dev(hipStream_t st, const float* logits, long long ld, const int* suppress, int n_sup,
                                           const int* begin_suppress, int n_beg, int* tokens, int ld_tok, int n_tok, int* last, int* done,
                                           int* alive, float* sum_logp, int R, int V, int* rec, int eos, int no_timestamps,
                                           int max_initial, const int* row_key, const int* serial) {
  F5E_REQUIRE(sum_logp && row_key && serial, "whisper_sample_pick_dev: null operand");
  const int rc = pick_dev_check("whisper_sample_pick_dev", logits, ld, suppress, n_sup, begin_suppress, n_beg, tokens, ld_tok,
                                n_tok, last, done, alive, rec, R, V, eos, 2);
  if (rc != F5E_OK) return rc;
  if (no_timestamps != -1) F5E_TS_DEV_REQUIRE("whisper_sample_pick_dev");   // -1: without the timestamp rules
  F5E_REQUIRE(max_initial >= -1, "whisper_sample_pick_dev: need max_initial >= -1 (got %d)", max_initial);
  hipLaunchKernelGGL(sample_pick_dev_kernel, dim3((unsigned)R), dim3(256), 0, st, logits, ld, suppress, n_sup, begin_suppress,
                     n_beg, tokens, ld_tok, n_tok, last, done, sum_logp, V, rec, eos, no_timestamps, max_initial, row_key, serial);
  hipLaunchKernelGGL(alive_advance_kernel, dim3(1), dim3(256), 0, st, done, alive, R, rec);
  F5E_LAUNCH_CHECK("whisper_sample_pick_dev");
  return F5E_OK;
}
