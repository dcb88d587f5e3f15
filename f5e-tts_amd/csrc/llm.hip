// The kernels of a Qwen2-style decoder-only language model (infer/qwen2.py): everything around the GEMMs, which are
// f5e_gemm_f32_w16 (prefill) and f5e_gemm_f32_w16_skinny (decode).  fp32 throughout, no allocation, no synchronisation, no
// floating-point atomics, no workgroup waits for another; every reduction runs in a fixed order, so a launch is reproducible
// and a row's result does not depend on its batch-mates.  What changes from token to token is read from the step record of
// whisper_step.hip (rec[0] = p, rec[2], rec[3] = the seed), so one decode step can be captured once and replayed.
//
//   f5e_rmsnorm_f32              y = (x * rsqrt(mean(x^2) + eps)) * w, one wave per row
//   f5e_swiglu_f32               out = silu(gate) * up from the fused gate | up projection
//   f5e_llm_embed_f32 / _w16     out[i] = table[ids[i]] (ids on the device: `last` of the decode step is the U = 1 form)
//   f5e_gqa_rope_append_f32      causal attention of U new positions behind p0 cached ones, rotary positions, grouped heads
//   f5e_gqa_rope_decode_dev_f32  one position from the step record, one workgroup per (row, key/value head)
//   f5e_llm_pick_dev             repetition penalty, temperature, top-k, top-p and an inverse-CDF draw (or the arg max)
//
// Rotation of a head x at position pos (cos, sin f32 [max_pos][dk / 2]; two products and one addition per element, the unit
// is built with -ffp-contract=off):
//   x'[d] = x[d] cos[pos][d] - x[d + dk/2] sin[pos][d]                      d <  dk/2
//   x'[d] = x[d] cos[pos][d - dk/2] + x[d - dk/2] sin[pos][d - dk/2]        d >= dk/2
#include "f5e_common.h"
#include "w_load.h"
#include "whisper_pick.h"
#include <type_traits>

namespace {

constexpr int LLM_MAX_D = 8192, LLM_MAX_POS = 4096, LLM_MAX_G = 8, LLM_MAX_K = 64, LLM_MAX_EOS = 4;
constexpr int DEC_NT = 512;   // threads of the decode attention's workgroup
constexpr int REC_P = 0, REC_SEED_LO = 2, REC_SEED_HI = 3;

inline int grid_for(size_t total) {
  size_t g = (total + 255) / 256;
  return (int)(g < 4096 ? (g ? g : 1) : 4096);
}

// ---- RMSNorm: a wave per row, lane l holds the quads l, l + 64, ... -------------------------------------------------------------
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* x, int ldx, const float* __restrict__ w, float* out, int ldo,
                                                      int M, int D, float eps) {
  const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;                             // uniform over the wave
  const float* xr = x + (size_t)m * ldx;
  float s = 0.f;
  for (int c = 4 * lane; c < D; c += 256) {
    const f32x4 v = *(const f32x4*)(xr + c);
    s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  s = wave_sum(s);
  const float rs = 1.0f / sqrtf(s / (float)D + eps);
  float* o = out + (size_t)m * ldo;
  for (int c = 4 * lane; c < D; c += 256) {       // a lane rewrites only what it read: out may be x
    const f32x4 v = *(const f32x4*)(xr + c);
    *(f32x4*)(o + c) = (v * rs) * *(const f32x4*)(w + c);
  }
}

// ---- SwiGLU ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float silu_exact(float x) { return x / (1.0f + expf(-x)); }

__global__ __launch_bounds__(256) void swiglu_kernel(const float* __restrict__ gu, int ld, float* __restrict__ out, int ldo, int M,
                                                     int I) {
  const int i4 = I / 4;
  const size_t total = (size_t)M * i4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % i4) * 4, m = (int)(i / i4);
    const f32x4 g = *(const f32x4*)(gu + (size_t)m * ld + c), u = *(const f32x4*)(gu + (size_t)m * ld + I + c);
    *(f32x4*)(out + (size_t)m * ldo + c) =
        f32x4{silu_exact(g.x) * u.x, silu_exact(g.y) * u.y, silu_exact(g.z) * u.z, silu_exact(g.w) * u.w};
  }
}

// ---- token gather -------------------------------------------------------------------------------------------------------------------
template <class WL>
__global__ __launch_bounds__(256) void llm_embed_kernel(const int* __restrict__ ids, const typename WL::elem* __restrict__ emb,
                                                        float* __restrict__ out, int n, int D, int table_rows) {
  const int d4 = D / 4;
  const size_t total = (size_t)n * d4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int c = (int)(i % d4) * 4, r = (int)(i / d4);
    const int id = min(max(ids[r], 0), table_rows - 1);
    *(f32x4*)(out + (size_t)r * D + c) = WL::load4(emb + (size_t)id * D + c);
  }
}

// ---- attention: U new positions behind p0 cached ones --------------------------------------------------------------------------------
struct GqaArgs {
  const float* qkv;
  float *kc, *vc, *out;
  const int* begin;
  const float *cos, *sin;
  long long row_stride;
  int ld_qkv, pos_stride, ldo, U, H, Hkv, p0, max_pos;
  float scale;
};

// A head's row in the MFMA operand layout (lane (c16, g) holds elements 16 j + 4 g + i), rotated: src = the head + 4 g, cs /
// sn = the position's table row + 4 g.
template <int NB>
__device__ __forceinline__ void rope_load(const float* src, const float* cs, const float* sn, f32x4 (&o)[NB]) {
  f32x4 x[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) x[j] = *(const f32x4*)(src + 16 * j);
#pragma unroll
  for (int j = 0; j < NB / 2; ++j) {
    const f32x4 c = *(const f32x4*)(cs + 16 * j), s = *(const f32x4*)(sn + 16 * j);
    o[j] = x[j] * c - x[j + NB / 2] * s;
    o[j + NB / 2] = x[j + NB / 2] * c + x[j] * s;
  }
}

// One 16-key tile of the online softmax (the tile of f5e_attn_append_f32): kf = this lane's key row, vrow(i) = the value row of
// key 4 g + i, + c16, vis[i]: key 4 g + i is visible to this lane's query.
template <int NB, class VRow>
__device__ __forceinline__ void gqa_tile(const f32x4 (&kf)[NB], VRow vrow, const bool (&vis)[4], const f32x4 (&qa)[NB],
                                         f32x4 (&acc)[NB], float& m_run, float& l_run, float scale) {
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) s0 = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j][i], qa[j][i], s0, 0, 0, 0);
  float p[4], mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[i] = vis[i] ? s0[i] * scale : -INFINITY;
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
    const float* vp = vrow(i);
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16 * j], p[i], acc[j], 0, 0, 0);
  }
}

// One wave per (16-query tile, query head, row).  Position j of row r is rotated at max(j - begin[r], 0).
template <int DK>
__global__ __launch_bounds__(64) void gqa_append_kernel(GqaArgs a) {
  constexpr int NB = DK / 16, HALF = DK / 2;
  const int lane = threadIdx.x, c16 = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, r = blockIdx.z;
  const int U = a.U, p0 = a.p0, G = a.H / a.Hkv, hk = h / G;
  const int koff = a.H * DK + hk * DK, voff = (a.H + a.Hkv) * DK + hk * DK, hc = hk * DK;
  const size_t row0 = (size_t)r * U;
  const int lo = a.begin ? min(max(a.begin[r], 0), p0 + U) : 0;      // the first visible position of the row
  const int lo_u = max(lo - p0, 0);                                  // ... among the new ones
  const int q_last = min(q0 + 15, U - 1);
  const int qr = min(q0 + c16, U - 1);                    // this lane's query (clamped: loads stay in bounds)
  const bool q_in = q0 + c16 < U, q_ok = q_in && p0 + qr >= lo;
  const long long cache_row = (long long)r * a.row_stride;

  f32x4 qa[NB];
  {
    const int pos = min(max(p0 + qr - lo, 0), a.max_pos - 1);
    const float* rowp = a.qkv + (row0 + qr) * a.ld_qkv + 4 * g;
    const float *cs = a.cos + (size_t)pos * HALF + 4 * g, *sn = a.sin + (size_t)pos * HALF + 4 * g;
    rope_load<NB>(rowp + h * DK, cs, sn, qa);
    if (q_in && h == hk * G) {                            // the group's first head files the tile's positions, padded ones included
      f32x4 kn[NB];
      rope_load<NB>(rowp + koff, cs, sn, kn);
      float* kd = a.kc + cache_row + (long long)(p0 + qr) * a.pos_stride + hc + 4 * g;
      float* vd = a.vc + cache_row + (long long)(p0 + qr) * a.pos_stride + hc + 4 * g;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        *(f32x4*)(kd + 16 * j) = kn[j];
        *(f32x4*)(vd + 16 * j) = *(const f32x4*)(rowp + voff + 16 * j);
      }
    }
  }
  f32x4 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  if (p0 + q_last >= lo) {
    // the cached keys lo .. p0-1, filed rotated: no causal mask (every new query lies behind them); only slots below p0 are read
    for (int kt = lo & ~15; kt < p0; kt += 16) {
      const int kr = min(kt + c16, p0 - 1);
      const float* kp = a.kc + cache_row + (long long)kr * a.pos_stride + hc + 4 * g;
      f32x4 kf[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) kf[j] = *(const f32x4*)(kp + 16 * j);
      bool vis[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kt + 4 * g + i;
        vis[i] = q_ok && key >= lo && key < p0;
      }
      gqa_tile<NB>(kf, [&](int i) {
        const int vr = min(kt + 4 * g + i, p0 - 1);
        return (const float*)(a.vc + cache_row + (long long)vr * a.pos_stride + hc + c16);
      }, vis, qa, acc, m_run, l_run, a.scale);
    }
    // the new keys lo_u .. u, from qkv, rotated as they are filed
    for (int kt = lo_u & ~15; kt <= q_last; kt += 16) {
      const int kr = min(kt + c16, U - 1);
      const int pos = min(max(p0 + kr - lo, 0), a.max_pos - 1);
      f32x4 kf[NB];
      rope_load<NB>(a.qkv + (row0 + kr) * a.ld_qkv + koff + 4 * g, a.cos + (size_t)pos * HALF + 4 * g,
                    a.sin + (size_t)pos * HALF + 4 * g, kf);
      bool vis[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = kt + 4 * g + i;
        vis[i] = q_ok && key >= lo_u && key <= qr;
      }
      gqa_tile<NB>(kf, [&](int i) {
        const int vr = min(kt + 4 * g + i, U - 1);
        return a.qkv + (row0 + vr) * a.ld_qkv + voff + c16;
      }, vis, qa, acc, m_run, l_run, a.scale);
    }
  }
  if (q_in) {
    const float inv = (q_ok && l_run > 0.f) ? 1.0f / l_run : 0.f;   // a query below begin[r]: zeros
    float* op = a.out + (row0 + q0 + c16) * a.ldo + h * DK + 4 * g;
#pragma unroll
    for (int j = 0; j < NB; ++j) *(f32x4*)(op + 16 * j) = acc[j] * inv;
  }
}

// ---- attention: one position from the step record ---------------------------------------------------------------------------------------
// One workgroup of DEC_NT = 512 threads per (key/value head, row) serves the G query heads of the group; GT = G rounded up to 1, 2, 4, 8
// (the heads beyond G are zeros and are not stored).  Three passes: scores (16 lanes per key, the key row straight to
// registers in whole cache lines, the G rotated queries from LDS), weights, context (a thread per channel and key group); every cached
// element is read once for all G heads.  Maxima, sums and partial contexts are merged through LDS in a fixed order.
template <int DK, int GT>
__global__ __launch_bounds__(DEC_NT) void gqa_decode_kernel(const float* __restrict__ qkv, int ld_qkv, float* kc, float* vc,
                                                         long long row_stride, int pos_stride, const int* __restrict__ begin,
                                                         const float* __restrict__ cos, const float* __restrict__ sin,
                                                         float* __restrict__ out, int ldo, int H, int Hkv, int P, int max_pos,
                                                         const int* __restrict__ rec, float scale) {
  extern __shared__ float sc[];                   // [G][P] scores, then weights
  constexpr int HALF = DK / 2, KG = DEC_NT / DK, NW = DEC_NT / 64;
  __shared__ __attribute__((aligned(16))) float qs[GT * DK];
  __shared__ __attribute__((aligned(16))) float knew[DK];
  __shared__ float vnew[DK], red[DEC_NT * GT], rmax[GT][NW], rsum[GT][NW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hk = blockIdx.x, r = blockIdx.y, G = H / Hkv;
  const int p = min(max(rec[REC_P], 0), P - 1);
  const int lo = begin ? min(max(begin[r], 0), p) : 0;
  const int pos = min(p - lo, max_pos - 1);
  const float* me = qkv + (long long)r * ld_qkv;
  const int koff = H * DK + hk * DK, voff = (H + Hkv) * DK + hk * DK;
  float* kbase = kc + (long long)r * row_stride + hk * DK;
  float* vbase = vc + (long long)r * row_stride + hk * DK;
  const float *cs = cos + (size_t)pos * HALF, *sn = sin + (size_t)pos * HALF;

  // the group's queries and the new key, rotated; the key and the value into slot [r][p]
  for (int e = tid; e < (GT + 1) * DK; e += DEC_NT) {
    const int gh = e / DK, d = e % DK;
    if (gh < GT && gh >= G) {
      qs[e] = 0.f;
      continue;
    }
    const float* src = gh < GT ? me + (hk * G + gh) * DK : me + koff;
    const int dd = d < HALF ? d : d - HALF;
    const float x = src[d], y = src[d < HALF ? d + HALF : d - HALF];
    const float val = d < HALF ? x * cs[dd] - y * sn[dd] : x * cs[dd] + y * sn[dd];
    if (gh < GT) {
      qs[e] = val;
    } else {
      knew[d] = val;
      kbase[(long long)p * pos_stride + d] = val;
    }
  }
  for (int d = tid; d < DK; d += DEC_NT) {
    const float v = me[voff + d];
    vnew[d] = v;
    vbase[(long long)p * pos_stride + d] = v;
  }
  __syncthreads();

  // ---- 1. scores
  float mx[GT];
#pragma unroll
  for (int gq = 0; gq < GT; ++gq) mx[gq] = -__builtin_inff();
  // LPK lanes share a key: lane `sub` of the group takes quads sub, sub + LPK, ... of the key row, so a group reads 16 LPK
  // consecutive bytes and a wave 64 / LPK whole key rows; the partial dot products are folded across the group (DPP inside a
  // 16-lane row; the 8-lane groups of dk = 32 take one shuffle), every lane of the group ends with the score.
  constexpr int LPK = DK / 4 < 16 ? DK / 4 : 16, NV = DK / 4 / LPK, KPB = DEC_NT / LPK;
  const int sub = tid % LPK, kq = tid / LPK;
  // NK keys of the group at once, j0, j0 + jstep, ...: every load is issued before the first product, so NK NV 16-byte loads
  // per lane are in flight (the launch is a handful of waves: what hides the memory latency is the loads per lane).  A key's
  // own arithmetic does not depend on NK.
  auto score = [&](auto nk, const float* kr0, long long kstep, int j0, int jstep) {
    constexpr int NK = decltype(nk)::value;
    f32x4 kv[NK][NV];
#pragma unroll
    for (int u = 0; u < NK; ++u)
#pragma unroll
      for (int v = 0; v < NV; ++v) kv[u][v] = *(const f32x4*)(kr0 + u * kstep + 4 * (sub + LPK * v));
#pragma unroll
    for (int u = 0; u < NK; ++u) {
      float acc[GT];
#pragma unroll
      for (int gq = 0; gq < GT; ++gq) acc[gq] = 0.f;
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const f32x4 k4 = kv[u][v];
#pragma unroll
        for (int gq = 0; gq < GT; ++gq) {
          const f32x4 q = *(const f32x4*)(qs + gq * DK + 4 * (sub + LPK * v));
          acc[gq] += q.x * k4.x + q.y * k4.y + q.z * k4.z + q.w * k4.w;
        }
      }
#pragma unroll
      for (int gq = 0; gq < GT; ++gq) {
        float a = add_xor2(add_xor1(acc[gq]));
        if constexpr (LPK == 16) {
          a += dpp_f32<0x124>(a);                 // row_ror:4
          a += dpp_f32<0x128>(a);                 // row_ror:8
        } else {
          a += __shfl_xor(a, 4, 64);
        }
        const float sv = a * scale;
        if (sub == 0 && gq < G) sc[gq * P + j0 + u * jstep] = sv;
        mx[gq] = fmaxf(mx[gq], sv);
      }
    }
  };
  {
    const long long kstep = (long long)KPB * pos_stride;
    int j = lo + kq;                              // uniform over a group
    for (; j + 7 * KPB < p; j += 8 * KPB) score(std::integral_constant<int, 8>{}, kbase + (long long)j * pos_stride, kstep, j, KPB);
    for (; j < p; j += KPB) score(std::integral_constant<int, 1>{}, kbase + (long long)j * pos_stride, 0, j, 0);
  }
  if ((p - lo) % KPB == kq) score(std::integral_constant<int, 1>{}, knew, 0, p, 0);   // the new key from LDS: no slot the launch writes is read
#pragma unroll
  for (int gq = 0; gq < GT; ++gq) {
    const float m = wave_max(mx[gq]);
    if (lane == 0) rmax[gq][wave] = m;
  }
  __syncthreads();
  float mg[GT], sum[GT];
#pragma unroll
  for (int gq = 0; gq < GT; ++gq) {
    mg[gq] = rmax[gq][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) mg[gq] = fmaxf(mg[gq], rmax[gq][w]);
    sum[gq] = 0.f;
  }
  // ---- 2. weights, a thread per key (the barrier above stands between the scores' writers and these readers)
  for (int j = lo + tid; j <= p; j += DEC_NT) {
#pragma unroll
    for (int gq = 0; gq < GT; ++gq)
      if (gq < G) {
        const float e = expf(sc[gq * P + j] - mg[gq]);
        sc[gq * P + j] = e;
        sum[gq] += e;
      }
  }
#pragma unroll
  for (int gq = 0; gq < GT; ++gq) {
    const float s = wave_sum(sum[gq]);
    if (lane == 0) rsum[gq][wave] = s;
  }
  __syncthreads();
  // ---- 3. context: thread (kg, d) takes the keys lo + kg, lo + kg + KG, ... of channel d
  const int kg = tid / DK, d = tid % DK;
  float acc[GT];
#pragma unroll
  for (int gq = 0; gq < GT; ++gq) acc[gq] = 0.f;
  {
    constexpr int NU = 16;                        // value loads in flight per lane; the sums keep the order of the keys
    int j = lo + kg;
    for (; j + (NU - 1) * KG < p; j += NU * KG) {
      float v[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u) v[u] = vbase[(long long)(j + u * KG) * pos_stride + d];
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int gq = 0; gq < GT; ++gq)
          if (gq < G) acc[gq] += sc[gq * P + j + u * KG] * v[u];
    }
    for (; j < p; j += KG) {
      const float v = vbase[(long long)j * pos_stride + d];
#pragma unroll
      for (int gq = 0; gq < GT; ++gq)
        if (gq < G) acc[gq] += sc[gq * P + j] * v;
    }
  }
  if ((p - lo) % KG == kg) {
    const float v = vnew[d];
#pragma unroll
    for (int gq = 0; gq < GT; ++gq)
      if (gq < G) acc[gq] += sc[gq * P + p] * v;
  }
#pragma unroll
  for (int gq = 0; gq < GT; ++gq) red[(kg * GT + gq) * DK + d] = acc[gq];
  __syncthreads();
  for (int e = tid; e < G * DK; e += DEC_NT) {
    const int gq = e / DK, dd = e % DK;
    float o = red[gq * DK + dd];
#pragma unroll
    for (int k = 1; k < KG; ++k) o += red[(k * GT + gq) * DK + dd];
    float tot = rsum[gq][0];
#pragma unroll
    for (int w = 1; w < NW; ++w) tot += rsum[gq][w];     // in wave order
    out[(long long)r * ldo + (hk * G + gq) * DK + dd] = o * (1.0f / tot);
  }
}

// ---- the pick ---------------------------------------------------------------------------------------------------------------------------
struct LlmPick {
  float penalty, temperature, top_p;
  int top_k, do_sample, n_eos, eos[LLM_MAX_EOS], pad;
};

// (value, id) as one word: a larger word is a larger value or, at equal values, a lower id.  Never 0.
__device__ __forceinline__ unsigned long long pick_word(float y, int v) {
  return ((unsigned long long)rank_key(y) << 32) | (unsigned long long)(0xffffffffu - (unsigned)v);
}
__device__ __forceinline__ float pick_value(unsigned long long w) {
  const unsigned k = (unsigned)(w >> 32);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ int pick_id(unsigned long long w) { return (int)(0xffffffffu - (unsigned)(w & 0xffffffffu)); }

// One workgroup per row.  The row is read once, in chunks of 1024 classes: a class that beats the k-th of the running list
// enters a candidate buffer (through a counter: its order there does not matter), and a chunk with candidates re-ranks list
// and candidates by counting; words are distinct, so ranks are, and the result does not depend on timing.  Thread 0 then
// walks the k survivors.
__global__ __launch_bounds__(256) void llm_pick_kernel(const float* __restrict__ logits, long long ld, int* tokens, int ld_tok,
                                                       int n_tok, const int* __restrict__ begin, int* last, int* done, int V,
                                                       const int* __restrict__ rec, LlmPick prm, const int* __restrict__ row_key,
                                                       const int* __restrict__ serial, int* __restrict__ keep_id,
                                                       float* __restrict__ keep_p, int* __restrict__ keep_n) {
  __shared__ unsigned bits[GP_MAX_V / 32];
  __shared__ unsigned long long cand[1024], top[LLM_MAX_K], ntop[LLM_MAX_K];
  __shared__ int cnt[2];                         // by the chunk's parity: a reset never meets the previous chunk's readers
  const int tid = threadIdx.x, r = blockIdx.x;
  const int p = min(max(rec[REC_P], 0), n_tok - 2);
  int* trow = tokens + (size_t)r * ld_tok;
  if (done[r]) {                                  // uniform over the workgroup
    if (tid == 0) {
      trow[p + 1] = prm.pad, last[r] = prm.pad;
      if (keep_n) keep_n[r] = 0;
    }
    return;
  }
  const int words = (V + 31) / 32;
  for (int i = tid; i < words; i += 256) bits[i] = 0u;
  if (tid < LLM_MAX_K) top[tid] = 0ull;
  __syncthreads();
  const int b = begin ? min(max(begin[r], 0), p) : 0;
  for (int i = b + tid; i <= p; i += 256) {       // the classes that occur in the row's tokens, prompt and generated alike
    const int v = trow[i];
    if (v >= 0 && v < V) atomicOr(&bits[v >> 5], 1u << (v & 31));
  }
  const int k = prm.do_sample ? prm.top_k : 1;
  const float* row = logits + (size_t)r * ld;
  for (int base = 0; base < V; base += 1024) {
    int* const cn = &cnt[(base >> 10) & 1];
    if (tid == 0) *cn = 0;
    __syncthreads();
    const unsigned long long thr = top[k - 1];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int v = base + 256 * q + tid;
      if (v < V) {
        float x = row[v];
        if ((bits[v >> 5] >> (v & 31)) & 1u) x = x < 0.f ? x * prm.penalty : x / prm.penalty;
        if (prm.do_sample) x = x / prm.temperature;
        const unsigned long long w = pick_word(x, v);
        if (w > thr) cand[atomicAdd(cn, 1)] = w;
      }
    }
    __syncthreads();
    const int n = *cn;
    if (n) {                                      // uniform
      if (tid < LLM_MAX_K) ntop[tid] = 0ull;
      __syncthreads();
      for (int e = tid; e < LLM_MAX_K + n; e += 256) {
        const unsigned long long w = e < LLM_MAX_K ? top[e] : cand[e - LLM_MAX_K];
        if (w == 0ull) continue;
        int rank = 0;
        for (int f = 0; f < LLM_MAX_K; ++f) rank += top[f] > w ? 1 : 0;
        for (int f = 0; f < n; ++f) rank += cand[f] > w ? 1 : 0;
        if (rank < k) ntop[rank] = w;
      }
      __syncthreads();
      if (tid < LLM_MAX_K) top[tid] = ntop[tid];  // the next round's barrier comes before its first read
    }
  }
  __syncthreads();
  if (tid != 0) return;
  float* ef = (float*)cand;                       // exp(y - y_max) of the survivors, descending
  int choice = 0, keep = 1;
  if (prm.do_sample) {
    const float y0 = pick_value(top[0]);
    float S = 0.f;
    for (int i = k - 1; i >= 0; --i) {            // ascending order of probability
      ef[i] = expf(pick_value(top[i]) - y0);
      S += ef[i];
    }
    keep = k;
    float cum = 0.f;
    const float cut = 1.0f - prm.top_p;
    for (int i = k - 1; i >= 1; --i) {            // TopPLogitsWarper: drop while the ascending cumulative sum is <= 1 - top_p
      cum += ef[i] / S;
      if (cum <= cut) keep = i;
      else break;
    }
    float S2 = 0.f;
    for (int i = 0; i < keep; ++i) S2 += ef[i];
    unsigned w4[4];
    philox4x32_10(0u, (unsigned)p, (unsigned)serial[r], (unsigned)row_key[r], (unsigned)rec[REC_SEED_LO], (unsigned)rec[REC_SEED_HI],
                  w4);
    const float u = ((float)(w4[0] >> 8) + 0.5f) * 0x1p-24f;
    const float target = u * S2;
    float c = 0.f;
    choice = keep - 1;
    for (int i = 0; i < keep; ++i) {
      c += ef[i];
      if (c >= target) {
        choice = i;
        break;
      }
    }
    if (keep_p)
      for (int i = 0; i < keep; ++i) keep_p[(size_t)r * LLM_MAX_K + i] = ef[i] / S2;
  } else if (keep_p) {
    keep_p[(size_t)r * LLM_MAX_K] = 1.0f;
  }
  if (keep_id)
    for (int i = 0; i < keep; ++i) keep_id[(size_t)r * LLM_MAX_K + i] = pick_id(top[i]);
  if (keep_n) keep_n[r] = keep;
  const int arg = pick_id(top[choice]);
  trow[p + 1] = arg;
  last[r] = arg;
  for (int i = 0; i < prm.n_eos; ++i)
    if (arg == prm.eos[i]) done[r] = 1;
}

// The rows still open, and the step's one writer of p: a single workgroup behind the pick, the step's last reader.
__global__ __launch_bounds__(256) void llm_alive_advance_kernel(const int* __restrict__ done, int* __restrict__ alive, int R,
                                                                int* rec) {
  __shared__ int red[4];
  const int n = alive_count_rows(done, R, red);
  if (threadIdx.x == 0) {
    *alive = n;
    const int p = rec[REC_P];
    rec[REC_P] = p < 0x7ffffffe ? p + 1 : p;
  }
}

#define LLM_UNSUPPORTED(cond, ...)   \
  do {                               \
    if (!(cond)) {                   \
      f5e_set_error(__VA_ARGS__);    \
      return F5E_ERR_UNSUPPORTED;    \
    }                                \
  } while (0)

int gqa_check(const char* name, const float* qkv, int ld_qkv, const float* kc, const float* vc, long long row_stride, int pos_stride,
              const float* cos, const float* sin, int max_pos, const float* out, int ldo, int R, int P, int H, int Hkv, int dk) {
  F5E_REQUIRE(qkv && kc && vc && out && cos && sin, "%s: null operand", name);
  F5E_REQUIRE(R > 0 && R <= 65535 && H > 0 && H <= 65535 && Hkv > 0 && H % Hkv == 0,
              "%s: need 0 < R, H <= 65535 and Hkv dividing H (R=%d H=%d Hkv=%d)", name, R, H, Hkv);
  LLM_UNSUPPORTED(dk == 32 || dk == 64 || dk == 128, "%s: head dim %d is not built (32, 64 and 128 are)", name, dk);
  LLM_UNSUPPORTED(H / Hkv <= LLM_MAX_G, "%s: %d query heads per key/value head, more than %d", name, H / Hkv, LLM_MAX_G);
  LLM_UNSUPPORTED(P > 0 && P <= LLM_MAX_POS, "%s: need 0 < cached positions <= %d (got %d)", name, LLM_MAX_POS, P);
  F5E_REQUIRE(max_pos >= P, "%s: the rotary tables hold %d positions, fewer than the %d cached ones", name, max_pos, P);
  const long long HQ = (long long)H * dk, HK = (long long)Hkv * dk;
  F5E_REQUIRE(ld_qkv >= HQ + 2 * HK && ldo >= HQ && pos_stride >= HK && row_stride >= (long long)(P - 1) * pos_stride + HK,
              "%s: a stride is smaller than the data it spans", name);
  F5E_REQUIRE(ld_qkv % 4 == 0 && ldo % 4 == 0 && pos_stride % 4 == 0 && row_stride % 4 == 0 &&
                  (((uintptr_t)qkv | (uintptr_t)kc | (uintptr_t)vc | (uintptr_t)out | (uintptr_t)cos | (uintptr_t)sin) & 15) == 0,
              "%s: strides must be multiples of 4 floats, qkv, kc, vc, out, cos and sin 16-byte aligned", name);
  return F5E_OK;
}

}  // namespace

extern "C" int f5e_rmsnorm_f32(hipStream_t st, const float* x, int ldx, const float* w, float* out, int ldo, int M, int D,
                               float eps) {
  F5E_REQUIRE(x && w && out, "rmsnorm_f32: null operand");
  F5E_REQUIRE(M > 0 && D > 0 && D % 4 == 0, "rmsnorm_f32: need M > 0 and D a positive multiple of 4 (M=%d D=%d)", M, D);
  LLM_UNSUPPORTED(D <= LLM_MAX_D, "rmsnorm_f32: D = %d exceeds %d", D, LLM_MAX_D);
  F5E_REQUIRE(ldx >= D && ldo >= D && ldx % 4 == 0 && ldo % 4 == 0 && (((uintptr_t)x | (uintptr_t)w | (uintptr_t)out) & 15) == 0,
              "rmsnorm_f32: row strides must be multiples of 4 floats and >= D, x, w and out 16-byte aligned");
  F5E_REQUIRE(eps >= 0.f, "rmsnorm_f32: eps must not be negative");
  hipLaunchKernelGGL(rmsnorm_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, x, ldx, w, out, ldo, M, D, eps);
  F5E_LAUNCH_CHECK("rmsnorm_f32");
  return F5E_OK;
}

extern "C" int f5e_swiglu_f32(hipStream_t st, const float* gu, int ld, float* out, int ldo, int M, int I) {
  F5E_REQUIRE(gu && out, "swiglu_f32: null operand");
  F5E_REQUIRE(M > 0 && I > 0 && I % 4 == 0, "swiglu_f32: need M > 0 and I a positive multiple of 4 (M=%d I=%d)", M, I);
  F5E_REQUIRE(ld >= 2LL * I && ldo >= I && ld % 4 == 0 && ldo % 4 == 0 && (((uintptr_t)gu | (uintptr_t)out) & 15) == 0,
              "swiglu_f32: need ld >= 2 I, ldo >= I, both multiples of 4 floats, gu and out 16-byte aligned");
  hipLaunchKernelGGL(swiglu_kernel, dim3(grid_for((size_t)M * I / 4)), dim3(256), 0, st, gu, ld, out, ldo, M, I);
  F5E_LAUNCH_CHECK("swiglu_f32");
  return F5E_OK;
}

template <class WL>
static int llm_embed_launch(const char* name, hipStream_t st, const int* ids, const void* emb, int emb_align, float* out, int n, int D,
                            int table_rows) {
  F5E_REQUIRE(ids && emb && out, "%s: null operand", name);
  F5E_REQUIRE(n > 0 && D > 0 && D % 4 == 0 && table_rows > 0, "%s: need n > 0, D a multiple of 4 and a non-empty table (n=%d D=%d)",
              name, n, D);
  F5E_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)emb & (uintptr_t)(emb_align - 1)) == 0,
              "%s: out must be 16-byte aligned, emb 16-byte (a 16-bit emb: 8-byte)", name);
  hipLaunchKernelGGL(llm_embed_kernel<WL>, dim3(grid_for((size_t)n * D / 4)), dim3(256), 0, st, ids,
                     (const typename WL::elem*)emb, out, n, D, table_rows);
  F5E_LAUNCH_CHECK(name);
  return F5E_OK;
}

extern "C" int f5e_llm_embed_f32(hipStream_t st, const int* ids, const float* emb, float* out, int n, int D, int table_rows) {
  return llm_embed_launch<WLoadF32>("llm_embed_f32", st, ids, emb, 16, out, n, D, table_rows);
}

extern "C" int f5e_llm_embed_w16(hipStream_t st, const int* ids, const void* emb, int wtype, float* out, int n, int D,
                                 int table_rows) {
  F5E_REQUIRE(wtype == F5E_W_FP16 || wtype == F5E_W_BF16, "llm_embed_w16: wtype %d is neither F5E_W_FP16 nor F5E_W_BF16", wtype);
  if (wtype == F5E_W_FP16) return llm_embed_launch<WLoad16<F5E_W_FP16>>("llm_embed_w16", st, ids, emb, 8, out, n, D, table_rows);
  return llm_embed_launch<WLoad16<F5E_W_BF16>>("llm_embed_w16", st, ids, emb, 8, out, n, D, table_rows);
}

extern "C" int f5e_gqa_rope_append_f32(hipStream_t st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                                       int pos_stride, const int* begin, const float* cos, const float* sin, int max_pos, float* out,
                                       int ldo, int R, int U, int Umax, int H, int Hkv, int dk, int p0, float scale) {
  const int rc = gqa_check("gqa_rope_append_f32", qkv, ld_qkv, kc, vc, row_stride, pos_stride, cos, sin, max_pos, out, ldo, R, Umax, H,
                           Hkv, dk);
  if (rc != F5E_OK) return rc;
  F5E_REQUIRE(U >= 1 && p0 >= 0 && (long long)p0 + U <= Umax,
              "gqa_rope_append_f32: need U >= 1, p0 >= 0 and p0 + U <= Umax (p0=%d U=%d Umax=%d)", p0, U, Umax);
  const GqaArgs a{qkv, kc, vc, out, begin, cos, sin, row_stride, ld_qkv, pos_stride, ldo, U, H, Hkv, p0, max_pos, scale};
  const dim3 grid((unsigned)((U + 15) / 16), (unsigned)H, (unsigned)R);
  switch (dk) {
    case 32: hipLaunchKernelGGL(gqa_append_kernel<32>, grid, dim3(64), 0, st, a); break;
    case 64: hipLaunchKernelGGL(gqa_append_kernel<64>, grid, dim3(64), 0, st, a); break;
    default: hipLaunchKernelGGL(gqa_append_kernel<128>, grid, dim3(64), 0, st, a); break;
  }
  F5E_LAUNCH_CHECK("gqa_rope_append_f32");
  return F5E_OK;
}

template <int DK, int GT>
static int gqa_decode_launch(hipStream_t st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride, int pos_stride,
                             const int* begin, const float* cos, const float* sin, int max_pos, float* out, int ldo, int R, int P,
                             int H, int Hkv, const int* rec, float scale) {
  static F5eDeviceOnce once;
  F5E_OPT_IN_LDS(once, (gqa_decode_kernel<DK, GT>), LLM_MAX_G * LLM_MAX_POS * 4);
  const int lds = (H / Hkv) * P * 4;
  hipLaunchKernelGGL((gqa_decode_kernel<DK, GT>), dim3((unsigned)Hkv, (unsigned)R), dim3(DEC_NT), lds, st, qkv, ld_qkv, kc, vc,
                     row_stride, pos_stride, begin, cos, sin, out, ldo, H, Hkv, P, max_pos, rec, scale);
  F5E_LAUNCH_CHECK("gqa_rope_decode_dev_f32");
  return F5E_OK;
}

extern "C" int f5e_gqa_rope_decode_dev_f32(hipStream_t st, const float* qkv, int ld_qkv, float* kc, float* vc, long long row_stride,
                                           int pos_stride, const int* begin, const float* cos, const float* sin, int max_pos,
                                           float* out, int ldo, int R, int P, int H, int Hkv, int dk, const int* rec, float scale) {
  const int rc = gqa_check("gqa_rope_decode_dev_f32", qkv, ld_qkv, kc, vc, row_stride, pos_stride, cos, sin, max_pos, out, ldo, R, P,
                           H, Hkv, dk);
  if (rc != F5E_OK) return rc;
  F5E_REQUIRE(rec && ((uintptr_t)rec & 15) == 0, "gqa_rope_decode_dev_f32: the step record must be 16-byte aligned and not null");
  const int G = H / Hkv, gt = G <= 1 ? 1 : G <= 2 ? 2 : G <= 4 ? 4 : 8;
#define LLM_DEC_GO(DK, GT)                                                                                                     \
  return gqa_decode_launch<DK, GT>(st, qkv, ld_qkv, kc, vc, row_stride, pos_stride, begin, cos, sin, max_pos, out, ldo, R, P, H, \
                                   Hkv, rec, scale)
#define LLM_DEC_DK(DK)          \
  switch (gt) {                 \
    case 1: LLM_DEC_GO(DK, 1);  \
    case 2: LLM_DEC_GO(DK, 2);  \
    case 4: LLM_DEC_GO(DK, 4);  \
    default: LLM_DEC_GO(DK, 8); \
  }
  switch (dk) {
    case 32: LLM_DEC_DK(32);
    case 64: LLM_DEC_DK(64);
    default: LLM_DEC_DK(128);
  }
#undef LLM_DEC_DK
#undef LLM_DEC_GO
}

extern "C" int f5e_llm_pick_dev(hipStream_t st, const float* logits, long long ld, int* tokens, int ld_tok, int n_tok,
                                const int* begin, int* last, int* done, int* alive, int R, int V, int* rec, int do_sample,
                                float penalty, float temperature, int top_k, float top_p, const int* eos_host, int n_eos, int pad,
                                const int* row_key, const int* serial, int* keep_id, float* keep_p, int* keep_n) {
  F5E_REQUIRE(logits && tokens && last && done && alive && rec, "llm_pick_dev: null operand");
  F5E_REQUIRE(((uintptr_t)rec & 15) == 0, "llm_pick_dev: the step record must be 16-byte aligned");
  LLM_UNSUPPORTED(V >= 2 && V <= GP_MAX_V, "llm_pick_dev: need 2 <= V <= %d (V=%d)", GP_MAX_V, V);
  F5E_REQUIRE(R > 0 && R <= 0x7fffffff / 2 && ld >= V, "llm_pick_dev: need R > 0 and ld >= V (R=%d V=%d)", R, V);
  F5E_REQUIRE(n_tok >= 2 && ld_tok >= n_tok, "llm_pick_dev: token rows need 2 <= n_tok <= ld_tok columns (n_tok=%d ld_tok=%d)", n_tok,
              ld_tok);
  F5E_REQUIRE(penalty >= 1.f && penalty < __builtin_inff(), "llm_pick_dev: need a finite repetition penalty >= 1");
  F5E_REQUIRE(n_eos >= 0 && n_eos <= LLM_MAX_EOS && (n_eos == 0 || eos_host) && pad >= 0 && pad < V,
              "llm_pick_dev: need at most %d eos ids and 0 <= pad < V (n_eos=%d pad=%d)", LLM_MAX_EOS, n_eos, pad);
  LlmPick prm{penalty, 1.f, 1.f, 1, do_sample ? 1 : 0, n_eos, {-1, -1, -1, -1}, pad};
  for (int i = 0; i < n_eos; ++i) {
    F5E_REQUIRE(eos_host[i] >= 0 && eos_host[i] < V, "llm_pick_dev: need 0 <= eos < V (eos[%d]=%d)", i, eos_host[i]);
    prm.eos[i] = eos_host[i];
  }
  if (do_sample) {
    F5E_REQUIRE(row_key && serial, "llm_pick_dev: sampling needs row_key and serial");
    F5E_REQUIRE(temperature > 0.f && temperature < __builtin_inff() && top_p > 0.f && top_p <= 1.f,
                "llm_pick_dev: need a finite temperature > 0 and 0 < top_p <= 1");
    LLM_UNSUPPORTED(top_k >= 1 && top_k <= LLM_MAX_K && top_k <= V, "llm_pick_dev: need 1 <= top_k <= min(%d, V) (top_k=%d)",
                    LLM_MAX_K, top_k);
    prm.temperature = temperature, prm.top_p = top_p, prm.top_k = top_k;
  }
  hipLaunchKernelGGL(llm_pick_kernel, dim3((unsigned)R), dim3(256), 0, st, logits, ld, tokens, ld_tok, n_tok, begin, last, done, V,
                     rec, prm, row_key, serial, keep_id, keep_p, keep_n);
  hipLaunchKernelGGL(llm_alive_advance_kernel, dim3(1), dim3(256), 0, st, done, alive, R, rec);
  F5E_LAUNCH_CHECK("llm_pick_dev");
  return F5E_OK;
}
