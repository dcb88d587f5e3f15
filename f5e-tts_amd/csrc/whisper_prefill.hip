// Whisper's decoder prefill: a prompt of U positions per row goes through every layer in ONE pass (conditioning on the
// previous windows' text and an initial prompt put up to max_target_positions / 2 tokens in front of the first pick), instead
// of U rounds of the cached single-position step.  fp32 throughout.
//
//   f5e_attn_prefill_f32   causal self-attention of positions 0 .. U-1 of R rows from the fused projection q | k | v, against
//                          themselves, which also files k and v in the layer's caches (slots [r][0 .. U-1]).  The wave tile
//                          of attn_f32_kernel (ppg_attention.hip): one wave per (row, head, 16-query tile), S^T = K . Q^T and
//                          O^T = V^T . P^T on v_mfma_f32_16x16x4_f32, so that no accumulator changes lanes.  Keys and values
//                          are read from qkv, never from the caches, so a launch reads nothing that it writes; the tile that
//                          owns 16 positions of a head stores their k and v (a lane's float4 of the q load, 2 D and D further
//                          on).  begin[r]: a row left-padded to the common length sees keys begin[r] .. i only; a query below
//                          begin[r] yields zeros.
//   f5e_whisper_embed      x[r][u] = emb[ids[r][u]] + pos[max(p0 + u - begin[r], 0)]: the position table shifted per row
//                          (f5e_text_gather indexes it by u alone).  U = 1 with p0 = p is the decode step's form.
//
// The decode step that follows a padded prompt, f5e_attn_decode_from_f32, is attn_decode_kernel's FROM instantiation
// (attn_decode.hip).
#include "f5e_common.h"
#include "w_load.h"

namespace {

struct PrefillArgs {
  const float* qkv;
  float *kc, *vc, *out;
  const int* begin;
  long long row_stride;
  int ld_qkv, pos_stride, ldo, U, HD;
  float scale;
};

template <int DK>
__global__ __launch_bounds__(64) void attn_prefill_kernel(PrefillArgs a) {
  constexpr int NB = DK / 16;
  const int lane = threadIdx.x, c16 = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, hd = blockIdx.y, r = blockIdx.z;
  const int U = a.U, hc = hd * DK;
  const size_t row0 = (size_t)r * U;
  const int lo = a.begin ? min(max(a.begin[r], 0), U) : 0;
  const int q_last = min(q0 + 15, U - 1);
  const int qr = min(q0 + c16, U - 1);                    // this lane's query row (clamped: loads stay in bounds)
  const bool q_in = q0 + c16 < U, q_ok = q_in && qr >= lo;
  const int hi_q = q_ok ? qr + 1 : 0;                     // this row sees keys [lo, hi_q)
  const int t_lo = lo & ~15, t_hi = q_last >= lo ? q_last + 1 : 0;

  f32x4 qa[NB];
  {
    const float* qp = a.qkv + (row0 + qr) * a.ld_qkv + hc + 4 * g;
    float* kd = a.kc + (long long)r * a.row_stride + (long long)qr * a.pos_stride + hc + 4 * g;
    float* vd = a.vc + (long long)r * a.row_stride + (long long)qr * a.pos_stride + hc + 4 * g;
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

  for (int kt = t_lo; kt < t_hi; kt += 16) {
    const int kr = min(kt + c16, U - 1);                  // key row of the score product's A operand
    const float* kp = a.qkv + (row0 + kr) * a.ld_qkv + a.HD + hc + 4 * g;
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
      const int key = kt + 4 * g + i;
      p[i] = (key >= lo && key < hi_q) ? s0[i] * a.scale : -INFINITY;
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
      const int vr = min(kt + 4 * g + i, U - 1);
      const float* vp = a.qkv + (row0 + vr) * a.ld_qkv + 2 * a.HD + hc + c16;
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * j], p[i], acc[j], 0, 0, 0);
    }
  }
  if (q_in) {
    const float inv = (q_ok && l_run > 0.f) ? 1.0f / l_run : 0.f;   // a query below begin[r]: zeros
    float* op = a.out + (row0 + q0 + c16) * a.ldo + hc + 4 * g;
#pragma unroll
    for (int j = 0; j < NB; ++j) *(f32x4*)(op + 16 * j) = acc[j] * inv;
  }
}

template <class WL>   // the token table's loader (w_load.h): fp32, or 16-bit widened in registers
__global__ void whisper_embed_kernel(const int* __restrict__ ids, const int* __restrict__ begin,
                                     const typename WL::elem* __restrict__ emb, const float* __restrict__ pos, float* __restrict__ out, int R, int U, int D, int p0,
                                     int max_pos, int table_rows) {
  const int d4 = D / 4;
  const size_t total = (size_t)R * U * d4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % d4) * 4;
    const size_t ru = i / d4;
    const int u = (int)(ru % U), r = (int)(ru / U);
    // ids are validated on the host where they start there; the clamp keeps a bad id handed over as a device tensor from
    // reading outside the table (as f5e_text_gather)
    const int id = min(max(ids[ru], 0), table_rows - 1);
    const int at = min(max(p0 + u - (begin ? begin[r] : 0), 0), max_pos - 1);
    *(f32x4*)(out + ru * D + c) = WL::load4(emb + (size_t)id * D + c) + *(const f32x4*)(pos + (size_t)at * D + c);
  }
}

inline int grid_for(size_t total) {
  size_t g = (total + 255) / 256;
  return (int)(g < 4096 ? (g ? g : 1) : 4096);
}

}  // namespace

int f5e_attn_prefill_f32(hipStream_t st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                         int pos_stride, const int* begin, float* out, int ldo, int R, int U, int Umax, int H, int dk,
                         float scale) {
  F5E_REQUIRE(qkv && kc && vc && out, "attn_prefill_f32: null operand");
  F5E_REQUIRE(R > 0 && R <= 65535 && H > 0 && H <= 65535, "attn_prefill_f32: need 0 < R, H <= 65535");
  F5E_REQUIRE(dk == 16 || dk == 32 || dk == 64 || dk == 128, "attn_prefill_f32: head dim %d is not built (16, 32, 64 and 128 are)",
              dk);
  F5E_REQUIRE(Umax > 0 && Umax <= 4096 && U >= 1 && U <= Umax, "attn_prefill_f32: need 1 <= U <= Umax <= 4096 (U=%d Umax=%d)", U,
              Umax);
  const long long HD = (long long)H * dk;
  F5E_REQUIRE(ld_qkv >= 3 * HD && ldo >= HD && pos_stride >= HD && row_stride >= (long long)(Umax - 1) * pos_stride + HD,
              "attn_prefill_f32: a stride is smaller than the data it spans");
  F5E_REQUIRE(ld_qkv % 4 == 0 && ldo % 4 == 0 && pos_stride % 4 == 0 && row_stride % 4 == 0 &&
                  (((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)out) & 15) == 0,
              "attn_prefill_f32: strides must be multiples of 4 floats, qkv, kc, vc and out 16-byte aligned");
  const PrefillArgs a{qkv, kc, vc, out, begin, row_stride, ld_qkv, pos_stride, ldo, U, (int)HD, scale};
  const dim3 grid((unsigned)((U + 15) / 16), (unsigned)H, (unsigned)R);
  switch (dk) {
    case 16: hipLaunchKernelGGL(attn_prefill_kernel<16>, grid, dim3(64), 0, st, a); break;
    case 32: hipLaunchKernelGGL(attn_prefill_kernel<32>, grid, dim3(64), 0, st, a); break;
    case 64: hipLaunchKernelGGL(attn_prefill_kernel<64>, grid, dim3(64), 0, st, a); break;
    default: hipLaunchKernelGGL(attn_prefill_kernel<128>, grid, dim3(64), 0, st, a); break;
  }
  F5E_LAUNCH_CHECK("attn_prefill_f32");
  return F5E_OK;
}

template <class WL>
int whisper_embed_launch(const char* name, hipStream_t st, const int* ids, const int* begin, const void* emb, int emb_align,
                         const float* pos, float* out, int R, int U, int D, int p0, int max_pos, int table_rows) {
  F5E_REQUIRE(ids && emb && pos && out, "%s: null operand", name);
  F5E_REQUIRE(R > 0 && U > 0 && D > 0 && D % 4 == 0 && table_rows > 0 && max_pos > 0 && p0 >= 0 && (long long)p0 + U <= max_pos,
              "%s: need R, U > 0, D a multiple of 4 and positions p0 .. p0 + U - 1 inside the table (p0=%d U=%d "
              "max_pos=%d)", name, p0, U, max_pos);
  F5E_REQUIRE((((uintptr_t)pos | (uintptr_t)out) & 15) == 0 && ((uintptr_t)emb & (uintptr_t)(emb_align - 1)) == 0,
              "%s: emb, pos and out must be 16-byte aligned (a 16-bit emb: 8-byte)", name);
  hipLaunchKernelGGL(whisper_embed_kernel<WL>, dim3(grid_for((size_t)R * U * D / 4)), dim3(256), 0, st, ids, begin,
                     (const typename WL::elem*)emb, pos, out, R, U, D, p0, max_pos, table_rows);
  F5E_LAUNCH_CHECK(name);
  return F5E_OK;
}

int f5e_whisper_embed(hipStream_t st, const int* ids, const int* begin, const float* emb, const float* pos, float* out, int R,
                      int U, int D, int p0, int max_pos, int table_rows) {
  return whisper_embed_launch<WLoadF32>("whisper_embed", st, ids, begin, emb, 16, pos, out, R, U, D, p0, max_pos, table_rows);
}

int f5e_whisper_embed_w16(hipStream_t st, const int* ids, const int* begin, const void* emb, int wtype, const float* pos,
                          float* out, int R, int U, int D, int p0, int max_pos, int table_rows) {
  F5E_REQUIRE(wtype == F5E_W_FP16 || wtype == F5E_W_BF16, "whisper_embed_w16: wtype %d is neither F5E_W_FP16 nor F5E_W_BF16", wtype);
  if (wtype == F5E_W_FP16)
    return whisper_embed_launch<WLoad16<F5E_W_FP16>>("whisper_embed_w16", st, ids, begin, emb, 8, pos, out, R, U, D, p0, max_pos,
                                                     table_rows);
  return whisper_embed_launch<WLoad16<F5E_W_BF16>>("whisper_embed_w16", st, ids, begin, emb, 8, pos, out, R, U, D, p0, max_pos,
                                                   table_rows);
}
