// Fused relative-position attention of the wenet Conformer (ppg/wenet/transformer/attention.py:172-222, the variant
// without rel_shift: the position term is indexed by the KEY's absolute position), exact fp32, with an optional chunk
// band (wenet/utils/mask.py subsequent_chunk_mask): the kernel behind the chunk-by-chunk streaming mode of the PPG
// extractor (encoder.py:210-355), where a query in chunk c = t / chunk sees keys [max(0, (c - left) chunk), (c + 1) chunk).
//
//   f5e_relpos_attn   out[q, h] = softmax_k(((q+u)_h . k_h[k] + (q+v)_h . p_h[k]) * scale) . v_h over the query's band
//   f5e_relbias_attn_f32   WavLM's self-attention (gated relative-position bias, computed on the fly from a [H][2 Tt - 1] table):
//                     out[q, h] = softmax_k(q_h . k_h[k] * scale + gate[b][h][q] * table[h][k - q + Tt - 1]) . v_h, keys < kv_len[b]
//
// One wave per (sequence, head, 16-query tile), no LDS.  Everything is computed TRANSPOSED on v_mfma_f32_16x16x4_f32 so
// that no accumulator ever changes lanes:
//   S^T [key][query] = K . (Q+u)^T + P . (Q+v)^T     A = K / P rows (m = key), B = query rows (n = query); C/D puts the
//                                                     query on the lane (col = lane & 15) and keys 4 g + r (g = lane >> 4)
//                                                     in register r: the row softmax is 4 registers + two xor-shuffles
//   O^T [d][query]   = V^T . P^T                      k-step r takes keys {4 g + r}: its B operand IS register r of the
//                                                     probabilities, its A operand one V element per lane
// The k index of the score products is permuted the same way on both operands (a lane's float4 covers d = 16 j + 4 g + 0..3,
// element r feeds k-slot g of step (j, r)), which leaves the sum unchanged up to fp32 summation order.
// Key tiles outside the union of the tile's row bands are skipped; inside it, keys outside a row's own band are masked.
#include "f5e_common.h"

namespace {

// One argument block for all entry points.  f5e_relpos_attn: Tq == Tk == T, pos and D (= H dk, the offset of the q + v half
// of a qu row) set, causal unused.  f5e_mha_f32: pos / D / chunk / left unused, q_begin 0.  f5e_relbias_attn_f32: as f5e_mha_f32
// without causal, Tq == Tk, plus gate [B][H][Tq], table [H][2 Tt - 1] and Tt >= Tq.
struct AttnArgs {
  const float *q, *k, *pos, *v;
  float* out;
  const int* kv_len;
  int ldq, ldk, ldp, ldv, ldo;
  int Tq, Tk, D, q_begin, chunk, left, causal;
  float scale;
  const float *gate, *table;
  int Tt;
};

enum { ATTN_PLAIN = 0, ATTN_RELPOS = 1, ATTN_RELBIAS = 2 };

// The wave tile.  RELPOS: the second score product (q + v) . p, the chunk band, and a query at or beyond the key length
// yields zeros.  Otherwise (f5e_mha_f32, the attention decoder's self- and source attention, attention.py:79-111): the band
// of query i is [0, min(i + 1, len)) when causal and [0, len) otherwise, so a query below the key length is NOT required:
// every query row is computed, and one with no visible key yields zeros (the reference's masked_fill after the softmax).
// RELBIAS: the band is [0, len) for every query below len; a query at or beyond len yields zeros (as RELPOS).  The bias of
// register r is ONE gather from the head's table at key - query + Tt - 1, scaled by the query's gate.
template <int DK, int MODE>
__global__ __launch_bounds__(64) void attn_f32_kernel(AttnArgs a) {
  constexpr bool RELPOS = MODE == ATTN_RELPOS, RELBIAS = MODE == ATTN_RELBIAS;
  constexpr int NB = DK / 16;
  const int lane = threadIdx.x, c16 = lane & 15, g = lane >> 4;
  const int q0 = a.q_begin + blockIdx.x * 16, hd = blockIdx.y, b = blockIdx.z;
  const int len = a.kv_len ? min(max(a.kv_len[b], 0), a.Tk) : a.Tk;
  const size_t rowq = (size_t)b * a.Tq, rowk = (size_t)b * a.Tk;
  const int hc = hd * DK;
  const int q_last = min(q0 + 15, a.Tq - 1);
  const int qr = min(q0 + c16, a.Tq - 1);                 // this lane's query row (clamped: loads stay in bounds)
  const bool q_in = q0 + c16 < a.Tq;
  // band of this lane's row: keys [lo_q, hi_q); of the tile (the union of its rows' bands, 16-aligned): [t_lo, t_hi)
  bool q_ok;
  int lo_q, hi_q, t_lo, t_hi;
  if constexpr (RELPOS) {
    // band of local row r: [lo(r), hi(r)); both are monotonic in r, so the tile's union is [lo(first row), hi(last row))
    auto band_lo = [&](int r) { return (a.chunk <= 0 || a.left < 0) ? 0 : max(0, (r / a.chunk - a.left) * a.chunk); };
    auto band_hi = [&](int r) { return a.chunk <= 0 ? len : min((r / a.chunk + 1) * a.chunk, len); };
    q_ok = q_in && q0 + c16 < len;
    lo_q = band_lo(qr), hi_q = q_ok ? band_hi(qr) : 0;
    t_lo = band_lo(q0) & ~15, t_hi = q0 < len ? band_hi(q_last) : 0;
  } else if constexpr (RELBIAS) {
    q_ok = q_in && q0 + c16 < len;
    lo_q = 0, hi_q = q_ok ? len : 0;
    t_lo = 0, t_hi = q0 < len ? len : 0;
  } else {
    q_ok = q_in;
    lo_q = 0, hi_q = q_ok ? (a.causal ? min(qr + 1, len) : len) : 0;
    t_lo = 0, t_hi = a.causal ? min(q_last + 1, len) : len;
  }
  float gq = 0.f;
  const float* tab = nullptr;
  if constexpr (RELBIAS) {
    gq = a.gate[((size_t)b * gridDim.y + hd) * a.Tq + qr];
    tab = a.table + (size_t)hd * (2 * a.Tt - 1);
  }

  f32x4 qa[NB], qb[RELPOS ? NB : 1];
  {
    const float* qp = a.q + (rowq + qr) * a.ldq + hc + 4 * g;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      qa[j] = *(const f32x4*)(qp + 16 * j);
      if constexpr (RELPOS) qb[j] = *(const f32x4*)(qp + a.D + 16 * j);
    }
  }
  f32x4 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  for (int kt = t_lo; kt < t_hi; kt += 16) {
    const int kr = min(kt + c16, len - 1);               // key row of the score product's A operand (len > 0 here)
    const float* kp = a.k + (rowk + kr) * a.ldk + hc + 4 * g;
    const float* pp = RELPOS ? a.pos + (size_t)kr * a.ldp + hc + 4 * g : nullptr;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const f32x4 kf = *(const f32x4*)(kp + 16 * j);
      f32x4 pf = {0.f, 0.f, 0.f, 0.f};
      if constexpr (RELPOS) pf = *(const f32x4*)(pp + 16 * j);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[r], qa[j][r], s0, 0, 0, 0);
        if constexpr (RELPOS) s1 = __builtin_amdgcn_mfma_f32_16x16x4f32(pf[r], qb[j][r], s1, 0, 0, 0);
      }
    }
    float p[4], mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = kt + 4 * g + r;
      const bool seen = key >= lo_q && key < hi_q;
      if constexpr (RELPOS) p[r] = seen ? (s0[r] + s1[r]) * a.scale : -INFINITY;
      else if constexpr (RELBIAS) {
        const int ti = min(max(key - qr + a.Tt - 1, 0), 2 * a.Tt - 2);   // a seen key is in range; the clamp is for the others
        p[r] = seen ? s0[r] * a.scale + gq * tab[ti] : -INFINITY;
      } else p[r] = seen ? s0[r] * a.scale : -INFINITY;
      mx = fmaxf(mx, p[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    const float m_use = m_new == -INFINITY ? 0.f : m_new;     // a row with nothing visible yet: exp(-inf - 0) = 0
    const float alpha = __expf(m_run - m_use);
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      p[r] = __expf(p[r] - m_use);
      sum += p[r];
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    l_run = l_run * alpha + sum;
    m_run = m_new;
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] *= alpha;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int vr = min(kt + 4 * g + r, len - 1);
      const float* vp = a.v + (rowk + vr) * a.ldv + hc + c16;
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * j], p[r], acc[j], 0, 0, 0);
    }
  }
  if (q_in) {
    const float inv = (q_ok && l_run > 0.f) ? 1.0f / l_run : 0.f;   // no visible key (RELPOS: or a row beyond the keys): zeros
    float* op = a.out + (rowq + q0 + c16) * a.ldo + hc + 4 * g;
#pragma unroll
    for (int j = 0; j < NB; ++j) *(f32x4*)(op + 16 * j) = acc[j] * inv;
  }
}

template <int MODE>
void launch_attn(hipStream_t st, const AttnArgs& a, int H, int B, int dk) {
  const dim3 grid((unsigned)((a.Tq - a.q_begin + 15) / 16), (unsigned)H, (unsigned)B);
  switch (dk) {
    case 16: hipLaunchKernelGGL((attn_f32_kernel<16, MODE>), grid, dim3(64), 0, st, a); break;
    case 32: hipLaunchKernelGGL((attn_f32_kernel<32, MODE>), grid, dim3(64), 0, st, a); break;
    case 64: hipLaunchKernelGGL((attn_f32_kernel<64, MODE>), grid, dim3(64), 0, st, a); break;
    default: hipLaunchKernelGGL((attn_f32_kernel<128, MODE>), grid, dim3(64), 0, st, a); break;
  }
}

}  // namespace

extern "C" int f5e_relpos_attn(hipStream_t st, const float* qu, int ldq, const float* k, int ldk, const float* pos, int ldp,
                               const float* v, int ldv, float* out, int ldo, const int* kv_len, int B, int T, int H, int dk,
                               int q_begin, int chunk, int left_chunks, float scale) {
  F5E_REQUIRE(qu && k && pos && v && out, "relpos_attn: null operand");
  F5E_REQUIRE(dk == 16 || dk == 32 || dk == 64 || dk == 128,
              "relpos_attn: head dim %d is not built (16, 32, 64 and 128 are)", dk);
  const long long D = (long long)H * dk;
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && H > 0 && H <= 65535 && q_begin >= 0 && q_begin < T,
              "relpos_attn: bad shape (B=%d T=%d H=%d q_begin=%d)", B, T, H, q_begin);
  F5E_REQUIRE(ldq >= 2 * D && ldk >= D && ldp >= D && ldv >= D && ldo >= D && ldq % 4 == 0 && ldk % 4 == 0 &&
                  ldp % 4 == 0 && ldo % 4 == 0,
              "relpos_attn: row strides must cover the heads (qu: 2 H dk) and be multiples of 4 floats");
  F5E_REQUIRE((((uintptr_t)qu | (uintptr_t)k | (uintptr_t)pos | (uintptr_t)out) & 15) == 0,
              "relpos_attn: qu, k, pos and out must be 16-byte aligned");
  const AttnArgs a{qu, k, pos, v, out, kv_len, ldq, ldk, ldp, ldv, ldo, T, T, (int)D, q_begin, chunk, left_chunks, 0, scale};
  launch_attn<ATTN_RELPOS>(st, a, H, B, dk);
  F5E_LAUNCH_CHECK("relpos_attn");
  return F5E_OK;
}

extern "C" int f5e_mha_f32(hipStream_t st, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, float* out,
                           int ldo, const int* kv_len, int B, int Tq, int Tk, int H, int dk, int causal, float scale) {
  F5E_REQUIRE(q && k && v && out, "mha_f32: null operand");
  F5E_REQUIRE(dk == 16 || dk == 32 || dk == 64 || dk == 128, "mha_f32: head dim %d is not built (16, 32, 64 and 128 are)", dk);
  const long long D = (long long)H * dk;
  F5E_REQUIRE(B > 0 && B <= 65535 && Tq > 0 && Tk > 0 && H > 0 && H <= 65535, "mha_f32: bad shape (B=%d Tq=%d Tk=%d H=%d)", B,
              Tq, Tk, H);
  F5E_REQUIRE(!causal || Tq == Tk, "mha_f32: causal needs Tq == Tk (got %d and %d)", Tq, Tk);
  F5E_REQUIRE(ldq >= D && ldk >= D && ldv >= D && ldo >= D && ldq % 4 == 0 && ldk % 4 == 0 && ldo % 4 == 0,
              "mha_f32: row strides must cover the heads (H dk) and those of q, k and out be multiples of 4 floats");
  F5E_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)out) & 15) == 0, "mha_f32: q, k and out must be 16-byte aligned");
  const AttnArgs a{q, k, nullptr, v, out, kv_len, ldq, ldk, 0, ldv, ldo, Tq, Tk, 0, 0, 0, -1, causal ? 1 : 0, scale};
  launch_attn<ATTN_PLAIN>(st, a, H, B, dk);
  F5E_LAUNCH_CHECK("mha_f32");
  return F5E_OK;
}

extern "C" int f5e_relbias_attn_f32(hipStream_t st, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                    float* out, int ldo, const float* gate, const float* table, int Tt, const int* kv_len, int B,
                                    int T, int H, int dk, float scale) {
  F5E_REQUIRE(q && k && v && out && gate && table, "relbias_attn_f32: null operand");
  F5E_REQUIRE(dk == 16 || dk == 32 || dk == 64, "relbias_attn_f32: head dim %d is not built (16, 32 and 64 are)", dk);
  const long long D = (long long)H * dk;
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && H > 0 && H <= 65535 && Tt >= T && Tt <= (1 << 29),
              "relbias_attn_f32: bad shape (B=%d T=%d H=%d Tt=%d; the table must cover Tt >= T)", B, T, H, Tt);
  F5E_REQUIRE(ldq >= D && ldk >= D && ldv >= D && ldo >= D && ldq % 4 == 0 && ldk % 4 == 0 && ldo % 4 == 0,
              "relbias_attn_f32: row strides must cover the heads (H dk) and those of q, k and out be multiples of 4 floats");
  F5E_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)out) & 15) == 0, "relbias_attn_f32: q, k and out must be 16-byte aligned");
  AttnArgs a{q, k, nullptr, v, out, kv_len, ldq, ldk, 0, ldv, ldo, T, T, 0, 0, 0, -1, 0, scale};
  a.gate = gate, a.table = table, a.Tt = Tt;
  launch_attn<ATTN_RELBIAS>(st, a, H, B, dk);
  F5E_LAUNCH_CHECK("relbias_attn_f32");
  return F5E_OK;
}
