// The body of the cached single-query self-attention, written once: f5e_attn_decode_f32 / f5e_attn_decode_from_f32
// (attn_decode.hip) hand it the step's position p from a kernel argument, f5e_attn_decode_dev_f32 (whisper_step.hip) from the
// step record on the device.  One wave per (row, head) = (blockIdx.y, blockIdx.x); see attn_decode.hip for the three passes.
#pragma once
#include "f5e_common.h"

constexpr int DEC_MAX_U = 4096;    // cached positions per row (the LDS score row of the attention wave)

template <int DK, bool FROM>
__device__ __forceinline__ void attn_decode_body(const float* __restrict__ qkv, int ld_qkv, float* kc, float* vc,
                                                 long long row_stride, int pos_stride, const int* __restrict__ anc, int ld_anc,
                                                 float* __restrict__ out, int ldo, int R, int H, int p, float scale,
                                                 const int* __restrict__ begin) {
  __shared__ float s[DEC_MAX_U];
  constexpr int G = DK >= 64 ? 1 : 64 / DK;     // key groups of the context pass
  constexpr int DPL = DK > 64 ? DK / 64 : 1;    // channels per lane of the context pass
  const int lane = threadIdx.x, h = blockIdx.x, r = blockIdx.y;
  const int HD = H * DK;
  const float* me = qkv + (long long)r * ld_qkv + h * DK;   // q; k at + HD, v at + 2 HD
  const long long head = (long long)h * DK;
  const int lo = FROM ? min(max(begin[r], 0), p) : 0;       // the first visible position

  // the new key / value into slot [r][p]
  for (int d = lane; d < DK; d += 64) {
    const long long o = (long long)r * row_stride + (long long)p * pos_stride + head + d;
    kc[o] = me[HD + d];
    vc[o] = me[2 * HD + d];
  }

  f32x4 q[DK / 4];
#pragma unroll
  for (int i = 0; i < DK / 4; ++i) q[i] = *(const f32x4*)(me + 4 * i);

  // ---- 1. scores
  float m = -__builtin_inff();
  for (int j = lo + lane; j <= p; j += 64) {
    const float* kr;
    if (j == p) {
      kr = me + HD;
    } else {
      const int src = anc ? min(max(anc[(long long)r * ld_anc + j], 0), R - 1) : r;   // the clamp keeps garbage in bounds
      kr = kc + (long long)src * row_stride + (long long)j * pos_stride + head;
    }
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < DK / 4; ++i) {
      const f32x4 kv = *(const f32x4*)(kr + 4 * i);
      acc += q[i].x * kv.x + q[i].y * kv.y + q[i].z * kv.z + q[i].w * kv.w;
    }
    acc *= scale;
    s[j] = acc;
    m = fmaxf(m, acc);
  }
  m = wave_max(m);
  // ---- 2. weights (a lane rewrites only the entries it wrote)
  float sum = 0.f;
  for (int j = lo + lane; j <= p; j += 64) {
    const float e = expf(s[j] - m);
    s[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  __syncthreads();
  // ---- 3. context
  const int g = DK >= 64 ? 0 : lane / DK, d0 = DK >= 64 ? lane : lane % DK;
  float acc[DPL];
#pragma unroll
  for (int i = 0; i < DPL; ++i) acc[i] = 0.f;
  for (int j = lo + g; j <= p; j += G) {
    const float* vr;
    if (j == p) {
      vr = me + 2 * HD;
    } else {
      const int src = anc ? min(max(anc[(long long)r * ld_anc + j], 0), R - 1) : r;
      vr = vc + (long long)src * row_stride + (long long)j * pos_stride + head;
    }
    const float w = s[j];
#pragma unroll
    for (int i = 0; i < DPL; ++i) acc[i] += w * vr[d0 + 64 * i];
  }
#pragma unroll
  for (int o = 32; o >= DK; o >>= 1) acc[0] += __shfl_xor(acc[0], o, 64);   // fold the key groups (DK < 64 only)
  if (g == 0) {
    const float inv = 1.f / sum;
#pragma unroll
    for (int i = 0; i < DPL; ++i) out[(long long)r * ldo + head + d0 + 64 * i] = acc[i] * inv;
  }
}
