// The online-softmax step of the flash-attention kernels (attention.hip, joint_attention.hip): one 64-key step of a
// wave's 32 queries in the checked form (row sums against ROWSUM_LIMIT, running maximum moved when needed), the unchecked
// fast form, and the end-of-pass finiteness test.  The arithmetic and its rationale are in attention.hip's header.
#pragma once
#include "f5e_common.h"

namespace {

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

constexpr float ROWSUM_LIMIT = 16777216.0f;   // 2^24, see the header: a step whose partial row sum exceeds it is redone

// One 64-key step of the online softmax for a wave's 32 queries (lane = query ql, key half hh).
//   qk(st, c): st[t] = c + (scores of keys 64 step + 32 t + ..., log2 domain), t = 0, 1 -- the 8 MFMAs of the step; may be
//              called twice (slow path), so the K fragments must still be at hand
//   on return st holds p = exp2(score - m_run) for the step's valid keys (0 for keys >= kv_len), l_val this lane's
//   running partial row sum, (m_run, minit, oacc) updated if the running maximum moved.
template <class QK>
__device__ __forceinline__ void softmax_step(QK&& qk, bool first, bool partial, int key_base, int kv_len, f32x16 (&st)[2],
                                             f32x16& minit, float& m_run, float& l_val, f32x16 (&oacc)[2]) {
  auto mask_tail = [&]() {
    // only the last step of a sequence: a real branch (the empty asm keeps hipcc from if-converting the block into 32
    // compares + 32 selects executed on EVERY step)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (key_base + t * 32 + (r & 3) + 8 * (r >> 2) >= kv_len) st[t][r] = -INFINITY;
  };
  if (!first) {
    qk(st, minit);                       // score - m_run
    if (partial) mask_tail();
    // ONE accumulation chain on purpose: two independent chains are SLP-packed into v_pk_add_f32, which costs more issue
    // time beside MFMAs than the two v_add_f32 it replaces (cdna guide, cycle constants: packed f32 VALU is an anti-lever)
    float rs = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[t][r] = fast_exp2(st[t][r]);
        rs += st[t][r];
      }
    if (__builtin_amdgcn_ballot_w64(!(rs <= ROWSUM_LIMIT)) == 0) {   // wave-uniform; NaN / inf fail the comparison
      l_val += rs;
      return;
    }
  }
  // slow path: the first step of a query tile, or some query of the wave met scores far above its m_run
  f32x16 zero;
#pragma unroll
  for (int r = 0; r < 16; ++r) zero[r] = 0.f;
  qk(st, zero);
  if (partial) mask_tail();
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[t][r]);
  mx = max_xor32(mx);                    // finite: every processed step holds at least one valid key
  const float m_new = fmaxf(m_run, mx);
  const float alpha = fast_exp2(m_run - m_new);   // first step: exp2(-inf) = 0
  l_val *= alpha;
  m_run = m_new;
#pragma unroll
  for (int r = 0; r < 16; ++r) { oacc[0][r] *= alpha; oacc[1][r] *= alpha; minit[r] = -m_new; }
  float rs = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[t][r] = fast_exp2(st[t][r] - m_new);
      rs += st[t][r];
    }
  l_val += rs;
}

// The unchecked step (see the header): scores arrive as score - m_run (C = minit), p = exp2 of them whatever their size --
// no maximum, no comparison, no branch.  Half 0's exp2 / row-sum VALU work is written between the two halves' MFMAs and
// half 1's between the P.V MFMAs, so that one wave keeps both pipes busy (a wave issues in order: VALU instructions placed
// behind a block of MFMAs wait for all of them to ISSUE, i.e. for the matrix pipe).
template <class KF, class VF>
__device__ __forceinline__ void fast_step(KF&& kfrag, VF&& vfrag, const bf16x8 (&qf)[4], const f32x16& minit, float& l_val,
                                          f32x16 (&oacc)[2]) {
  f32x16 s0, s1;
  s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfrag(0, 0), qf[0], minit, 0, 0, 0);
#pragma unroll
  for (int ks = 1; ks < 4; ++ks) s0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfrag(0, ks), qf[ks], s0, 0, 0, 0);
  s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfrag(1, 0), qf[0], minit, 0, 0, 0);
#pragma unroll
  for (int ks = 1; ks < 4; ++ks) s1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfrag(1, ks), qf[ks], s1, 0, 0, 0);
  float rs = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) { s0[r] = fast_exp2(s0[r]); rs += s0[r]; }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 8; ++j) pf[j] = (bf16)s0[8 * s + j];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag(0, s, dt), pf, oacc[dt], 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) { s1[r] = fast_exp2(s1[r]); rs += s1[r]; }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 8; ++j) pf[j] = (bf16)s1[8 * s + j];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vfrag(1, s, dt), pf, oacc[dt], 0, 0, 0);
  }
  l_val += rs;
}

// true when this lane's row sum and output accumulators are all finite (inf and NaN fail `<=`)
__device__ __forceinline__ bool accum_finite(float l_val, const f32x16 (&oacc)[2]) {
  float mag = fabsf(l_val);   // a SUM, not a maximum: fmaxf drops NaNs, an addition keeps them (and infinities)
#pragma unroll
  for (int r = 0; r < 16; ++r) mag += fabsf(oacc[0][r]) + fabsf(oacc[1][r]);
  return mag <= 3.0e38f;
}

}  // namespace
