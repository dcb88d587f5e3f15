// Joint audio-text attention of the MMDiT blocks (reference model/modules.py:647-718, JointAttnProcessor), head dim 64,
// bf16 in / bf16 out.  Per (sequence s, head h) the key / value set is the concatenation of two sequences, each with its
// own RoPE origin (applied by the two QKV GEMMs) and its own padding rule:
//
//   keys = audio keys 0 .. kv_len[s]-1  ++  text keys 0 .. Nt-1          (audio keys past kv_len[s] masked, text never)
//   o_x[s*N  + i][h*64 + d] = sum_key softmax_key(Qx[s,h,i,:] . K[key,:] / 8) V[key,d]     audio queries i < N
//   o_c[s*Nt + j][h*64 + d] = sum_key softmax_key(Qc[s,h,j,:] . K[key,:] / 8) V[key,d]     text queries  j < Nt
//
// Replaces the torch.cat of the two streams' q / k / v, the F.pad'ded key mask, F.scaled_dot_product_attention and the
// split of its output at modules.py:688-710.  f5e_flash_attn cannot express it: its mask is one key count per sequence
// over ONE fragment-major buffer, and padding the text segment into that buffer would leave unmasked zero keys inside the
// softmax.
//
// Operands: the fragment-major Q / K / V^T buffers that f5e_gemm_bf16_qkv_rope writes (layouts in attention.hip), one set
// per stream -- audio [S][H][n_pad_x][64] with rows_per_seq = N, text [S][H][n_pad_c][64] with rows_per_seq = Nt -- so the
// QKV GEMMs run unchanged, once per stream.  q arrives pre-scaled by log2(e) / 8 (scores in the log2 domain).
//
// Structure: attention.hip's LDS-free split-KV wave kernel (attn_fwd_kernel) with a two-segment key walk.  One wave = 32
// queries; the NSPLIT waves of a workgroup take the key steps wave, wave + NSPLIT, ... of the concatenated step list (the
// audio segment's ceil(kv_len / 64) 64-key steps, then the text segment's ceil(Nt / 64)) and merge (m, l, O) through LDS.
// Each segment's last step, when partial, masks its own tail in the checked form (softmax_step, attention_step.h); full
// steps of either segment run the unchecked fast_step.  The grid covers the audio q-tiles and, when o_c is set, the text
// q-tiles of every (sequence, head); both read the same K / V, so they share an XCD's L2 (same block order as
// attn_fwd_kernel).  The LDS-shared 128-query variant of f5e_flash_attn is not built here: large grids run this kernel
// unsplit.
//
// Numerics: m_run is the maximum of a wave's FIRST step, as in attn_fwd_kernel.  The text segment comes after the audio
// segment and can hold scores far above that step's; such a step leaves through the same paths as a late audio spike: a
// checked step (partial tail) trips the 2^24 row-sum limit and rescales, an unchecked one either stays finite (scale-free)
// or overflows exp2 to inf, which the end-of-pass accum_finite test catches and answers with a checked pass.
#include "attention_step.h"

namespace {

struct JointArgs {
  const bf16* qx; const bf16* kx; const bf16* vx;   // audio stream, [S][H][n_pad_x][64] fragment-major
  const bf16* qc; const bf16* kc; const bf16* vc;   // text stream,  [S][H][n_pad_c][64]
  bf16* ox; int ldo_x;
  bf16* oc; int ldo_c;                               // null: text queries skipped
  const int* kv_len;                                 // [S] audio key counts or null (= N)
  int S, H, N, n_pad_x, Nt, n_pad_c;
  int qtiles_x, qtiles;                              // audio q-tiles, all q-tiles per (sequence, head)
};

template <int NSPLIT>
__global__ __launch_bounds__(NSPLIT * 64, 2) void joint_attn_kernel(JointArgs a) {   // 2 waves per SIMD: <= 256 VGPRs
  // merge buffers: per extra wave, per lane: 32 O values + m + l
  __shared__ __attribute__((aligned(16))) float red[(NSPLIT > 1 ? NSPLIT - 1 : 1) * 64 * 34];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ql = lane & 31, hh = lane >> 5;

  // XCD-aware order (attn_fwd_kernel): all q-tiles of one (sequence, head), audio and text, on one XCD's L2
  int bid = blockIdx.x;
  {
    const int nblk = gridDim.x;
    const int q8 = nblk >> 3, r8 = nblk & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    bid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
  }
  const int qt_all = bid % a.qtiles;
  bid /= a.qtiles;
  const int head = bid % a.H;
  const int seq = bid / a.H;
  const size_t sh = (size_t)seq * a.H + head;
  const bool text_q = qt_all >= a.qtiles_x;
  const int qt = text_q ? qt_all - a.qtiles_x : qt_all;

  const int kv_x = a.kv_len ? min(max(a.kv_len[seq], 0), a.N) : a.N;   // valid audio keys
  const int na = (kv_x + 63) / 64;                                     // audio 64-key steps
  const int nsteps = na + (a.Nt + 63) / 64;                            // >= 1: text keys are never masked

  const bf16* Kx = a.kx + sh * a.n_pad_x * 64;
  const bf16* Vx = a.vx + sh * a.n_pad_x * 64;
  const bf16* Kc = a.kc + sh * a.n_pad_c * 64;
  const bf16* Vc = a.vc + sh * a.n_pad_c * 64;
  const bf16* Qg = text_q ? a.qc + sh * a.n_pad_c * 64 : a.qx + sh * a.n_pad_x * 64;

  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) qf[ks] = *(const bf16x8*)(Qg + ((size_t)(qt * 4 + ks) * 32 + ql) * 16 + hh * 8);

  // step t of the concatenated list: audio step t (t < na) or text step t - na
  bf16x8 kf[2][4], vf[2][2][2];   // [t32][ks], [t32][s16][dt]
  auto load_tile = [&](int t) {
    const bool txt = t >= na;
    const bf16* Kg = txt ? Kc : Kx;
    const bf16* Vg = txt ? Vc : Vx;
    const int t64 = txt ? t - na : t;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      const size_t tile = (size_t)t64 * 2 + t2;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) kf[t2][ks] = *(const bf16x8*)(Kg + ((tile * 4 + ks) * 32 + ql) * 16 + hh * 8);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          vf[t2][s][dt] = *(const bf16x8*)(Vg + ((((tile * 2 + s) * 2 + dt) * 32 + ql) * 2 + hh) * 8);
    }
  };

  f32x16 oacc[2], minit;
  float m_run, l_val;
  bf16x8 ck[2][4], cv[2][2][2];   // the current step's fragments (kf / vf already hold the next step's)
  int step;
  auto advance = [&]() -> int {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) ck[t][ks] = kf[t][ks];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) cv[t][s][dt] = vf[t][s][dt];
    }
    const int cur = step;
    step += NSPLIT;
    if (step < nsteps) load_tile(step);
    return cur;
  };
  auto pass_begin = [&]() {
#pragma unroll
    for (int r = 0; r < 16; ++r) { oacc[0][r] = 0.f; oacc[1][r] = 0.f; minit[r] = 0.f; }
    m_run = -INFINITY;
    l_val = 0.f;
    step = wave;
    if (step < nsteps) load_tile(step);
  };
  auto checked_tile = [&](bool first) {   // row sums checked against ROWSUM_LIMIT, running maximum moved when needed
    const int cur = advance();
    const bool txt = cur >= na;
    const int base = (txt ? cur - na : cur) * 64;   // first key of the step inside its segment
    const int lim = txt ? a.Nt : kv_x;              // the segment's valid keys
    f32x16 st[2];
    auto qk = [&](f32x16 (&d)[2], const f32x16& c) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        d[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ck[t][0], qf[0], c, 0, 0, 0);
#pragma unroll
        for (int ks = 1; ks < 4; ++ks) d[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ck[t][ks], qf[ks], d[t], 0, 0, 0);
      }
    };
    softmax_step(qk, first, base + 64 > lim, base + 4 * hh, lim, st, minit, m_run, l_val, oacc);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = (bf16)st[t][8 * s + j];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cv[t][s][dt], pf, oacc[dt], 0, 0, 0);
      }
  };
  auto fast_tile = [&]() {
    advance();
    auto kfrag = [&](int t, int ks) { return ck[t][ks]; };
    auto vfrag = [&](int t, int s, int dt) { return cv[t][s][dt]; };
    fast_step(kfrag, vfrag, qf, minit, l_val, oacc);
  };

  // Fast pass: the wave's first step establishes m_run; full steps of either segment run unchecked; each segment's
  // partial last step (its key mask) takes the checked form.  Steps ascend, so after a segment's full steps the wave is
  // either on that segment's partial step or past the segment.
  const int na_full = na * 64 > kv_x ? na - 1 : na;
  const int all_full = nsteps * 64 - na * 64 > a.Nt ? nsteps - 1 : nsteps;
  pass_begin();
  if (step < nsteps) checked_tile(true);
  while (step < na_full) fast_tile();
  if (step < na) checked_tile(false);        // audio tail: keys kv_len .. 64 na - 1 masked
  while (step < all_full) fast_tile();
  if (step < nsteps) checked_tile(false);    // text tail: keys Nt .. masked
  if (__builtin_amdgcn_ballot_w64(!accum_finite(l_val, oacc)) != 0) {   // wave-uniform; waves are independent until the merge
    pass_begin();
    bool first = true;
    while (step < nsteps) { checked_tile(first); first = false; }
  }

  float l_run = add_xor32(l_val);   // the two key halves of a query meet once, here
  // ---- merge the NSPLIT partial results (same queries, disjoint keys), as attn_fwd_kernel ----
  if (NSPLIT > 1) {
    if (wave > 0) {
      f32x4* dq = (f32x4*)(red + (wave - 1) * 64 * 34);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        dq[g * 64 + lane] = f32x4{oacc[0][4 * g], oacc[0][4 * g + 1], oacc[0][4 * g + 2], oacc[0][4 * g + 3]};
        dq[(4 + g) * 64 + lane] = f32x4{oacc[1][4 * g], oacc[1][4 * g + 1], oacc[1][4 * g + 2], oacc[1][4 * g + 3]};
      }
      *(f32x2*)(red + (wave - 1) * 64 * 34 + 64 * 32 + lane * 2) = f32x2{m_run, l_run};
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 1; w < NSPLIT; ++w) {
      const f32x4* sq = (const f32x4*)(red + (w - 1) * 64 * 34);
      const f32x2 ml = *(const f32x2*)(red + (w - 1) * 64 * 34 + 64 * 32 + lane * 2);
      const float m_new = fmaxf(m_run, ml[0]);
      // a wave that saw no step has m = -inf, l = 0, O = 0: factor exp2(-inf) = 0 (wave 0 always owns step 0)
      const float fa = fast_exp2(m_run - m_new), fb = fast_exp2(ml[0] - m_new);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 s0 = sq[g * 64 + lane], s1 = sq[(4 + g) * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          oacc[0][4 * g + r] = oacc[0][4 * g + r] * fa + s0[r] * fb;
          oacc[1][4 * g + r] = oacc[1][4 * g + r] * fa + s1[r] * fb;
        }
      }
      l_run = l_run * fa + ml[1] * fb;
      m_run = m_new;
    }
  }

  // ---- normalise + store through a row-major LDS image of the 32 x 64 tile (attn_fwd_kernel) ----
  {
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
    char* stg = (char*)red;
    if (NSPLIT > 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        *(bf16x4*)(stg + ql * 144 + 64 * dt + 16 * g + 8 * hh) =
            f2bf4(oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv, oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    bf16* o = text_q ? a.oc : a.ox;
    const int ldo = text_q ? a.ldo_c : a.ldo_x;
    const int rows = text_q ? a.Nt : a.N;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int r = it * 8 + (lane >> 3), c = lane & 7;
      const int q_row = qt * 32 + r;
      const uint4 v = *(const uint4*)(stg + r * 144 + c * 16);
      if (q_row < rows) *(uint4*)(o + ((size_t)seq * rows + q_row) * ldo + head * 64 + c * 8) = v;
    }
  }
}

}  // namespace

extern "C" int f5e_joint_attn(hipStream_t st, const void* qx, const void* kx, const void* vx, const void* qc,
                              const void* kc, const void* vc, void* o_x, int ldo_x, void* o_c, int ldo_c,
                              const int* kv_len, int S, int H, int N, int n_pad_x, int Nt, int n_pad_c, int splits) {
  F5E_REQUIRE(qx && kx && vx && kc && vc && o_x, "joint_attn: null pointer");
  F5E_REQUIRE(!o_c || qc, "joint_attn: o_c needs the text queries qc");
  F5E_REQUIRE(S > 0 && H > 0 && N > 0 && Nt > 0, "joint_attn: empty problem (S=%d H=%d N=%d Nt=%d)", S, H, N, Nt);
  F5E_REQUIRE(n_pad_x % 64 == 0 && n_pad_x >= N, "joint_attn: n_pad_x=%d must be a multiple of 64 and >= N=%d", n_pad_x, N);
  F5E_REQUIRE(n_pad_c % 64 == 0 && n_pad_c >= Nt, "joint_attn: n_pad_c=%d must be a multiple of 64 and >= Nt=%d", n_pad_c,
              Nt);
  F5E_REQUIRE(ldo_x % 8 == 0 && ldo_x >= H * 64 && ((uintptr_t)o_x & 15) == 0, "joint_attn: bad ldo_x=%d / o_x alignment",
              ldo_x);
  F5E_REQUIRE(!o_c || (ldo_c % 8 == 0 && ldo_c >= H * 64 && ((uintptr_t)o_c & 15) == 0),
              "joint_attn: bad ldo_c=%d / o_c alignment", ldo_c);
  JointArgs a{};
  a.qx = (const bf16*)qx; a.kx = (const bf16*)kx; a.vx = (const bf16*)vx;
  a.qc = (const bf16*)qc; a.kc = (const bf16*)kc; a.vc = (const bf16*)vc;
  a.ox = (bf16*)o_x; a.ldo_x = ldo_x; a.oc = (bf16*)o_c; a.ldo_c = ldo_c;
  a.kv_len = kv_len; a.S = S; a.H = H; a.N = N; a.n_pad_x = n_pad_x; a.Nt = Nt; a.n_pad_c = n_pad_c;
  a.qtiles_x = (N + 31) / 32;
  a.qtiles = a.qtiles_x + (o_c ? (Nt + 31) / 32 : 0);
  const long long grid_ll = (long long)a.qtiles * H * S;
  F5E_REQUIRE(grid_ll < (1LL << 31), "joint_attn: grid too large");
  const int grid = (int)grid_ll;
  if (splits <= 0) {
    // f5e_flash_attn_pf's rule over the grid of both query sets: the 4-way split while the grid is one round (up to 2
    // workgroups per CU), none past it; never more splits than key steps
    const int ksteps = (N + 63) / 64 + (Nt + 63) / 64;
    splits = grid > 2 * f5e_cu_count() ? 1 : 4;
    while (splits > 1 && splits > ksteps) splits >>= 1;
  }
  switch (splits) {
    case 1: hipLaunchKernelGGL(joint_attn_kernel<1>, dim3(grid), dim3(64), 0, st, a); break;
    case 2: hipLaunchKernelGGL(joint_attn_kernel<2>, dim3(grid), dim3(128), 0, st, a); break;
    case 4: hipLaunchKernelGGL(joint_attn_kernel<4>, dim3(grid), dim3(256), 0, st, a); break;
    default: F5E_REQUIRE(false, "joint_attn: splits must be 0 (auto), 1, 2 or 4");
  }
  F5E_LAUNCH_CHECK("joint_attn");
  return F5E_OK;
}
