// ECAPA-TDNN speaker-encoder head (reference eval/ecapa_tdnn.py, the half behind the WavLM hidden states): everything that
// is not a plain linear.  The 1x1 convolutions, the k5 input convolution (f5e_im2col) and the SE / pooling / tail linears
// run on f5e_gemm_f32, whose epilogue act(. + bias) * ch_scale + addend is conv -> ReLU -> BatchNorm(eval) and whose
// row_scale is the 0/1 frame mask written here by f5e_layer_mix_inorm.  Layouts: channels-last f32 [B][T][C]; all fp32.
// Ragged batches: frames t >= len[b] are ZERO in every tensor these kernels write and are left out of every statistic.
#include "f5e_common.h"
#include <math.h>

namespace {

constexpr int MIX_MAX_L = 256;
constexpr int RES2_TT = 16;         // output frames per workgroup of the Res2 chain (ops.RES2_TILE)
constexpr int RES2_MAX_LDS = 160 * 1024;

__device__ __forceinline__ int row_len(const int* len, int b, int T) {
  const int n = len ? len[b] : T;
  return n < 0 ? 0 : (n > T ? T : n);
}

// ---- f5e_layer_mix_inorm, launch 1: x[b][t][:] = sum_l softmax(fw)_l h_l[b][t][:] + 1e-6 (t < len, else 0); mask[b][t].
// One 16-byte column group per thread, up to 16 layers' loads in flight: the hidden states are read exactly once.
__global__ __launch_bounds__(256) void ecapa_layer_mix_kernel(const f32x4* __restrict__ hs, const float* __restrict__ fw,
                                                              const int* __restrict__ len, f32x4* __restrict__ x,
                                                              float* __restrict__ mask, int L, int T, int F4,
                                                              long long total) {
  __shared__ float sw[MIX_MAX_L];
  const int tid = threadIdx.x;
  if (tid < L) {
    float m = -INFINITY, s = 0.f;
    for (int l = 0; l < L; ++l) m = fmaxf(m, fw[l]);
    for (int l = 0; l < L; ++l) s += expf(fw[l] - m);
    sw[tid] = expf(fw[tid] - m) / s;
  }
  __syncthreads();
  const long long e = (long long)blockIdx.x * 256 + tid;
  if (e >= total) return;
  const long long bt = e / F4;
  const int f4 = (int)(e - bt * F4), b = (int)(bt / T), t = (int)(bt - (long long)b * T);
  const bool live = t < row_len(len, b, T);
  if (f4 == 0) mask[bt] = live ? 1.f : 0.f;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    for (int l0 = 0; l0 < L; l0 += 16) {      // 16 loads in flight per thread, summed in layer order
      f32x4 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (l0 + u < L) v[u] = __builtin_nontemporal_load(hs + (long long)(l0 + u) * total + e);
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (l0 + u < L) acc += v[u] * sw[l0 + u];
    }
    acc += 1e-6f;
  }
  x[e] = acc;
}

// RL row lanes x FL column groups (4 FL channels) per workgroup of 256: sum over the row lanes through LDS, result in every thread
template <int RL, int FL>
__device__ __forceinline__ f32x4 rows_sum(f32x4 v, f32x4* red, int tr, int fl) {
  __syncthreads();   // the previous use of red is over
  red[tr * FL + fl] = v;
  __syncthreads();
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < RL; ++r) s += red[r * FL + fl];
  return s;
}
__device__ __forceinline__ f32x4 rows32_sum(f32x4 v, f32x4* red, int tr, int fl) { return rows_sum<32, 8>(v, red, tr, fl); }

// ---- launch 2: InstanceNorm1d over t < len per (b, f), in place: biased variance about the mean, eps 1e-5, no affine.
__global__ __launch_bounds__(256) void ecapa_inorm_kernel(f32x4* __restrict__ x, const int* __restrict__ len, int T, int F4) {
  __shared__ f32x4 red[256];
  const int tid = threadIdx.x, fl = tid & 3, tr = tid >> 2, b = blockIdx.y;   // 64 row lanes x 16 channels (64-byte segments)
  const int f4 = blockIdx.x * 4 + fl;
  const bool on = f4 < F4;
  const int n = row_len(len, b, T);
  if (n == 0) return;
  f32x4* xb = x + (long long)b * T * F4 + (on ? f4 : 0);
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (on) for (int t = tr; t < n; t += 64) s += xb[(long long)t * F4];
  const f32x4 mean = rows_sum<64, 4>(s, red, tr, fl) / (float)n;
  f32x4 q = {0.f, 0.f, 0.f, 0.f};
  if (on) for (int t = tr; t < n; t += 64) { const f32x4 dlt = xb[(long long)t * F4] - mean; q += dlt * dlt; }
  const f32x4 var = rows_sum<64, 4>(q, red, tr, fl) / (float)n;
  f32x4 rstd;
#pragma unroll
  for (int i = 0; i < 4; ++i) rstd[i] = 1.0f / sqrtf(var[i] + 1e-5f);
  if (on) for (int t = tr; t < n; t += 64) xb[(long long)t * F4] = (xb[(long long)t * F4] - mean) * rstd;
}

// ---- f5e_res2_dconv: steps [first, first + count) of the Res2 chain in ONE launch.  A workgroup owns RES2_TT output frames
// of one batch row and recomputes a halo: LDS row r is frame t0 - count * d + r, R = RES2_TT + 2 * count * d rows; local step
// k is exact on rows [(k + 1) d, R - (k + 1) d), which is what step k + 1 reads.  Per step: In = Prev + x_i (zero outside
// [0, len)), the step's [w][3][w] weights into LDS (zero padded to 16 output / 4 input channels), then 16-frame x 16-channel
// tiles of v_mfma_f32_16x16x4_f32 over K = 3 taps x w, epilogue bn(relu(. + bias)) masked, into Prev and (own frames) y.
struct Res2Args {
  const float* x; int ldx;
  float* y; int ldy;
  const float* w;        // [7][w][3 * w], k = tap * w + ic
  const float* bias;     // [7][w]
  const float* scale;    // [7][w]  BatchNorm folded
  const float* shift;    // [7][w]
  const int* len;
  int T, wd, d, first, count, copy_last;
};

__global__ __launch_bounds__(256) void ecapa_res2_kernel(Res2Args a) {
  extern __shared__ f32x4 lds4[];
  float* lds = (float*)lds4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int b = blockIdx.y, t0 = blockIdx.x * RES2_TT, T = a.T, w = a.wd, d = a.d;
  const int wp = (w + 3) & ~3, ocp = (w + 15) & ~15, SS = wp + 4, KS = 3 * wp + 4;
  const int H = a.count * d, R = RES2_TT + 2 * H;
  float* In = lds;
  float* Prev = In + R * SS;
  float* Wl = Prev + R * SS;
  const int n = row_len(a.len, b, T);
  const float* xb = a.x + (size_t)b * T * a.ldx;
  float* yb = a.y + (size_t)b * T * a.ldy;

  for (int idx = tid; idx < R * wp; idx += 256) {
    const int r = idx / wp, ic = idx - r * wp, t = t0 - H + r;
    float v = 0.f;
    if (a.first > 0 && ic < w && t >= 0 && t < n) v = yb[(size_t)t * a.ldy + (a.first - 1) * w + ic];
    Prev[r * SS + ic] = v;
  }
  for (int k = 0; k < a.count; ++k) {
    const int i = a.first + k;
    __syncthreads();   // Prev complete (initial fill or the previous step's epilogue); In and Wl no longer read
    for (int idx = tid; idx < R * wp; idx += 256) {
      const int r = idx / wp, ic = idx - r * wp, t = t0 - H + r;
      float v = Prev[r * SS + ic];
      if (ic < w && t >= 0 && t < n) v += xb[(size_t)t * a.ldx + i * w + ic];
      In[r * SS + ic] = v;
    }
    const float* wi = a.w + (size_t)i * w * 3 * w;
    for (int idx = tid; idx < ocp * 3 * wp; idx += 256) {
      const int oc = idx / (3 * wp), kk = idx - oc * 3 * wp, j = kk / wp, ic = kk - j * wp;
      Wl[oc * KS + kk] = (oc < w && ic < w) ? wi[(size_t)oc * 3 * w + j * w + ic] : 0.f;
    }
    __syncthreads();
    const int lo = (k + 1) * d, hi = R - lo;
    const int nft = (hi - lo + 15) >> 4, noct = ocp >> 4;
    for (int u = wave; u < nft * noct; u += 4) {
      const int ft = u / noct, oct = u - ft * noct, r0 = lo + ft * 16;
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < 3; ++j) {
        const int rr = r0 + fr + (j - 1) * d;
        const bool ok = rr >= 0 && rr < R;
        const float* ap = In + (ok ? rr : 0) * SS + fq;
        const float* bp = Wl + (oct * 16 + fr) * KS + j * wp + fq;
        int ic0 = 0;
        for (; ic0 + 8 <= wp; ic0 += 8) {
          const float a0 = ok ? ap[ic0] : 0.f, a1 = ok ? ap[ic0 + 4] : 0.f;
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(bp[ic0], a0, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(bp[ic0 + 4], a1, acc1, 0, 0, 0);
        }
        if (ic0 < wp) acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(bp[ic0], ok ? ap[ic0] : 0.f, acc0, 0, 0, 0);
      }
      // acc[r]: output channel oct * 16 + fq * 4 + r of row r0 + fr (the operand map of gemm_f32.hip)
      const int row = r0 + fr, t = t0 - H + row;
      const bool live = row < hi && t >= 0 && t < n;
      const bool own = row >= H && row < H + RES2_TT && t < T;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int oc = oct * 16 + fq * 4 + r;
        if (oc >= w || row >= R) continue;
        const float z = acc0[r] + acc1[r] + a.bias[i * w + oc];
        const float v = live ? fmaxf(z, 0.f) * a.scale[i * w + oc] + a.shift[i * w + oc] : 0.f;
        Prev[row * SS + oc] = v;
        if (own) yb[(size_t)t * a.ldy + i * w + oc] = v;
      }
    }
  }
  if (a.copy_last)
    for (int idx = tid; idx < RES2_TT * w; idx += 256) {
      const int r = idx / w, c = idx - r * w, t = t0 + r;
      if (t < T) yb[(size_t)t * a.ldy + 7 * w + c] = t < n ? xb[(size_t)t * a.ldx + 7 * w + c] : 0.f;
    }
}

// The same chain for w a multiple of 16 with 16-byte aligned rows (the shipped encoders: w = 64): no channel padding, all
// global and LDS traffic in 16-byte accesses, and no staging pass between steps -- the epilogue of step k writes the next
// step's input (its result + x_{i+1}) straight into the other LDS image.  The step weights travel global -> registers -> LDS;
// those of step k + 1 are in flight while step k computes.  A lane reads 4 consecutive k of its row with one ds_read_b128 and
// feeds them to 4 MFMAs; both operands use the same k permutation, so every k is visited exactly once (as gemm_f32.hip).
constexpr int RES2_NT = 512;    // two waves per SIMD: one wave's ds_reads under the other's MFMAs
constexpr int RES2_WREG = 6;    // 16-byte weight chunks a thread carries: 512 * 6 * 4 floats = 64 x 192, i.e. w <= 64

template <int WC>   // the width when it is known at compile time (64: loops unrolled, divisions by constants), 0 = a.wd
__global__ __launch_bounds__(RES2_NT) void ecapa_res2_w16_kernel(Res2Args a) {
  extern __shared__ f32x4 lds4[];
  float* lds = (float*)lds4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int b = blockIdx.y, t0 = blockIdx.x * RES2_TT, T = a.T, w = WC ? WC : a.wd, d = a.d;
  constexpr int UN = WC ? WC / 16 : 1;
  const int SS = w + 4, KS = 3 * w + 4, w4 = w >> 2, rv = 3 * w4, nvec = w * rv;
  const int H = a.count * d, R = RES2_TT + 2 * H;
  float* cur = lds;
  float* nxt = cur + R * SS;
  float* Wl = nxt + R * SS;
  const int n = row_len(a.len, b, T);
  const float* xb = a.x + (size_t)b * T * a.ldx;
  float* yb = a.y + (size_t)b * T * a.ldy;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  f32x4 wreg[RES2_WREG];
  auto wload = [&](int i) {
    const f32x4* src = (const f32x4*)(a.w + (size_t)i * w * 3 * w);
#pragma unroll
    for (int v = 0; v < RES2_WREG; ++v) {
      const int idx = tid + v * RES2_NT;
      if (idx < nvec) wreg[v] = src[idx];
    }
  };
  auto wstore = [&](int i) {
    const f32x4* src = (const f32x4*)(a.w + (size_t)i * w * 3 * w);
#pragma unroll
    for (int v = 0; v < RES2_WREG; ++v) {
      const int idx = tid + v * RES2_NT;
      if (idx < nvec) { const int oc = idx / rv; *(f32x4*)(Wl + oc * KS + (idx - oc * rv) * 4) = wreg[v]; }
    }
    for (int idx = tid + RES2_WREG * RES2_NT; idx < nvec; idx += RES2_NT) {   // w > 64: the rest, not prefetched
      const int oc = idx / rv;
      *(f32x4*)(Wl + oc * KS + (idx - oc * rv) * 4) = src[idx];
    }
  };
  wload(a.first);
  for (int idx = tid; idx < R * w4; idx += RES2_NT) {      // input of the first step: y_{first-1} + x_first; the other image: 0
    const int r = idx / w4, c = (idx - r * w4) * 4, t = t0 - H + r;
    f32x4 v = zero4;
    if (t >= 0 && t < n) {
      v = *(const f32x4*)(xb + (size_t)t * a.ldx + a.first * w + c);
      if (a.first > 0) v += *(const f32x4*)(yb + (size_t)t * a.ldy + (a.first - 1) * w + c);
    }
    *(f32x4*)(cur + r * SS + c) = v;
    *(f32x4*)(nxt + r * SS + c) = zero4;
  }
  for (int k = 0; k < a.count; ++k) {
    const int i = a.first + k;
    const bool more = k + 1 < a.count;
    wstore(i);
    if (more) wload(i + 1);
    __syncthreads();   // Wl and cur complete
    const int lo = (k + 1) * d, hi = R - lo;
    const int nft = (hi - lo + 15) >> 4, noct = w >> 4;
    for (int u = wave; u < nft * noct; u += RES2_NT / 64) {
      const int ft = u / noct, oct = u - ft * noct, r0 = lo + ft * 16;
      // acc[r]: output channel oc0 + r of row r0 + fr (the operand map of gemm_f32.hip)
      const int row = r0 + fr, t = t0 - H + row, oc0 = oct * 16 + fq * 4;
      const bool live = row < hi && t >= 0 && t < n;
      f32x4 xn = zero4;
      if (more && live) xn = *(const f32x4*)(xb + (size_t)t * a.ldx + (i + 1) * w + oc0);
      const f32x4 bi = *(const f32x4*)(a.bias + i * w + oc0), sc = *(const f32x4*)(a.scale + i * w + oc0),
                  sh = *(const f32x4*)(a.shift + i * w + oc0);
      f32x4 acc0 = zero4, acc1 = zero4;
      for (int j = 0; j < 3; ++j) {
        const int rr = r0 + fr + (j - 1) * d;
        const bool ok = rr >= 0 && rr < R;
        const float* ap = cur + (ok ? rr : 0) * SS + fq * 4;
        const float* bp = Wl + (oct * 16 + fr) * KS + j * w + fq * 4;
#pragma clang loop unroll_count(UN)
        for (int ic0 = 0; ic0 < w; ic0 += 16) {
          f32x4 av = *(const f32x4*)(ap + ic0);
          const f32x4 bv = *(const f32x4*)(bp + ic0);
          if (!ok) av = zero4;
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[0], av[0], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[1], av[1], acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[2], av[2], acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[3], av[3], acc1, 0, 0, 0);
        }
      }
      if (row >= R) continue;
      f32x4 v = zero4;
      if (live) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc0[r] + acc1[r] + bi[r], 0.f) * sc[r] + sh[r];
      }
      *(f32x4*)(nxt + row * SS + oc0) = v + xn;
      if (row >= H && row < H + RES2_TT && t < T) *(f32x4*)(yb + (size_t)t * a.ldy + i * w + oc0) = v;
    }
    __syncthreads();   // every wave is done with cur and Wl; nxt complete
    float* sw = cur; cur = nxt; nxt = sw;
  }
  if (a.copy_last)
    for (int idx = tid; idx < RES2_TT * w4; idx += RES2_NT) {
      const int r = idx / w4, c = (idx - r * w4) * 4, t = t0 + r;
      if (t < T)
        *(f32x4*)(yb + (size_t)t * a.ldy + 7 * w + c) = t < n ? *(const f32x4*)(xb + (size_t)t * a.ldx + 7 * w + c) : zero4;
    }
}

// ---- f5e_time_stats: mean (and sqrt(unbiased variance + 1e-10)) over t < len per (b, c)
__global__ __launch_bounds__(256) void ecapa_time_stats_kernel(const float* __restrict__ x, int ldx, const int* __restrict__ len,
                                                               float* __restrict__ mean_out, float* __restrict__ std_out,
                                                               int ld_out, int T, int C4) {
  __shared__ f32x4 red[256];
  const int tid = threadIdx.x, fl = tid & 7, tr = tid >> 3, b = blockIdx.y;
  const int c4 = blockIdx.x * 8 + fl;
  const bool on = c4 < C4;
  const int n = row_len(len, b, T);
  const float* xb = x + (size_t)b * T * ldx + (on ? c4 : 0) * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (on) for (int t = tr; t < n; t += 32) s += *(const f32x4*)(xb + (size_t)t * ldx);
  const f32x4 mean = n > 0 ? rows32_sum(s, red, tr, fl) / (float)n : f32x4{0.f, 0.f, 0.f, 0.f};
  if (on && tr == 0) *(f32x4*)(mean_out + (size_t)b * ld_out + c4 * 4) = mean;
  if (!std_out) return;
  f32x4 q = {0.f, 0.f, 0.f, 0.f};
  if (on) for (int t = tr; t < n; t += 32) { const f32x4 dlt = *(const f32x4*)(xb + (size_t)t * ldx) - mean; q += dlt * dlt; }
  q = rows32_sum(q, red, tr, fl);
  if (on && tr == 0) {
    f32x4 sd;
#pragma unroll
    for (int i = 0; i < 4; ++i) sd[i] = sqrtf((n > 1 ? q[i] / (float)(n - 1) : 0.f) + 1e-10f);
    *(f32x4*)(std_out + (size_t)b * ld_out + c4 * 4) = sd;
  }
}

// ---- f5e_se_scale: out = x * sigmoid(gate[b]) + resid
__global__ __launch_bounds__(256) void ecapa_se_scale_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ gate,
                                                             const float* __restrict__ resid, int ldr, float* __restrict__ out,
                                                             int ldo, int T, int C4, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long long bt = e / C4;
  const int c = (int)(e - bt * C4) * 4, b = (int)(bt / T);
  const f32x4 g = *(const f32x4*)(gate + (size_t)b * C4 * 4 + c);
  const f32x4 v = *(const f32x4*)(x + (size_t)bt * ldx + c), r = *(const f32x4*)(resid + (size_t)bt * ldr + c);
  f32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = v[i] * (1.0f / (1.0f + expf(-g[i]))) + r[i];
  *(f32x4*)(out + (size_t)bt * ldo + c) = o;
}

// ---- f5e_bias_tanh: x[b][t][:] = tanh(x[b][t][:] + add[add_rows == 1 ? 0 : b][:]) in place
__global__ __launch_bounds__(256) void ecapa_bias_tanh_kernel(float* __restrict__ x, int ldx, const float* __restrict__ add,
                                                              int ld_add, int add_rows, int T, int N, long long total) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long long bt = e / N;
  const int j = (int)(e - bt * N), b = (int)(bt / T);
  float* p = x + (size_t)bt * ldx + j;
  *p = tanhf(*p + add[(size_t)(add_rows == 1 ? 0 : b) * ld_add + j]);
}

// ---- f5e_attn_stats_pool: one pass over t < len with an online softmax per (b, c); 32 row lanes merged through LDS.
// The second moment is carried about the running weighted mean (Welford's update with weights p = exp(l - running max)),
// not as sum alpha x^2 - mean^2: the same quantity without the cancellation, which at std << |mean| costs the sum-of-squares
// form a relative error of 2^-24 mean^2 / std^2.  A new maximum rescales the weight sum and the moment; the mean stays.
__global__ __launch_bounds__(256) void ecapa_pool_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ logit,
                                                         int ldl, const int* __restrict__ len, float* __restrict__ out, int T,
                                                         int C4) {
  __shared__ f32x4 red[4][256];
  const int tid = threadIdx.x, fl = tid & 7, tr = tid >> 3, b = blockIdx.y;
  const int c4 = blockIdx.x * 8 + fl;
  const bool on = c4 < C4;
  const int n = row_len(len, b, T);
  const float* xb = x + (size_t)b * T * ldx + (on ? c4 : 0) * 4;
  const float* lb = logit + (size_t)b * T * ldl + (on ? c4 : 0) * 4;
  f32x4 m, s = {0.f, 0.f, 0.f, 0.f}, mu = s, m2 = s;
  m[0] = m[1] = m[2] = m[3] = -INFINITY;
  if (on)
    for (int t = tr; t < n; t += 32) {
      const f32x4 l = *(const f32x4*)(lb + (size_t)t * ldl), v = *(const f32x4*)(xb + (size_t)t * ldx);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float mn = fmaxf(m[i], l[i]);
        const float c = expf(m[i] - mn), p = expf(l[i] - mn);   // m = -inf: c = 0
        const float sn = s[i] * c + p, dlt = v[i] - mu[i];
        mu[i] += dlt * (p / sn);
        m2[i] = m2[i] * c + p * dlt * (v[i] - mu[i]);
        s[i] = sn;
        m[i] = mn;
      }
    }
  red[0][tr * 8 + fl] = m; red[1][tr * 8 + fl] = s; red[2][tr * 8 + fl] = mu; red[3][tr * 8 + fl] = m2;
  __syncthreads();
  if (!on || tr != 0) return;
  f32x4 M = m;
  for (int r = 1; r < 32; ++r) {
    const f32x4 o = red[0][r * 8 + fl];
#pragma unroll
    for (int i = 0; i < 4; ++i) M[i] = fmaxf(M[i], o[i]);
  }
  f32x4 S = {0.f, 0.f, 0.f, 0.f}, MU = S, Q = S;
  for (int r = 0; r < 32; ++r) {
    const f32x4 mr = red[0][r * 8 + fl], sr = red[1][r * 8 + fl], ur = red[2][r * 8 + fl], qr = red[3][r * 8 + fl];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (mr[i] == -INFINITY) continue;             // a row lane without a frame
      const float c = expf(mr[i] - M[i]), w = sr[i] * c;
      const float sn = S[i] + w, dlt = ur[i] - MU[i];
      MU[i] += dlt * (w / sn);
      Q[i] += qr[i] * c + dlt * dlt * (S[i] * (w / sn));
      S[i] = sn;
    }
  }
  f32x4 sd;
#pragma unroll
  for (int i = 0; i < 4; ++i) sd[i] = sqrtf(fmaxf(n > 0 ? Q[i] / S[i] : 0.f, 1e-9f));
  float* ob = out + (size_t)b * C4 * 8;
  *(f32x4*)(ob + c4 * 4) = MU;
  *(f32x4*)(ob + C4 * 4 + c4 * 4) = sd;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int f5e_layer_mix_inorm(hipStream_t st, const float* hs, const float* feature_weight, const int* len, float* x, float* mask,
                        int L, int B, int T, int F) {
  F5E_REQUIRE(hs && feature_weight && x && mask, "layer_mix_inorm: null operand");
  F5E_REQUIRE(L > 0 && L <= MIX_MAX_L && B > 0 && B <= 65535 && T > 0 && F > 0 && F % 4 == 0,
              "layer_mix_inorm: need 0 < L <= %d, 0 < B <= 65535, T > 0 and F a positive multiple of 4", MIX_MAX_L);
  F5E_REQUIRE(al16(hs) && al16(x), "layer_mix_inorm: hs and x must be 16-byte aligned");
  const int F4 = F / 4;
  const long long total = (long long)B * T * F4;
  F5E_REQUIRE(total <= 0x7fffffffLL * 64, "layer_mix_inorm: B * T * F too large");
  hipLaunchKernelGGL(ecapa_layer_mix_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const f32x4*)hs,
                     feature_weight, len, (f32x4*)x, mask, L, T, F4, total);
  hipLaunchKernelGGL(ecapa_inorm_kernel, dim3((unsigned)((F4 + 3) / 4), (unsigned)B), dim3(256), 0, st, (f32x4*)x, len, T, F4);
  F5E_LAUNCH_CHECK("layer_mix_inorm");
  return F5E_OK;
}

int f5e_res2_dconv(hipStream_t st, const float* x, int ldx, float* y, int ldy, const float* w, const float* bias,
                   const float* scale, const float* shift, const int* len, int B, int T, int C, int dilation, int first,
                   int count) {
  F5E_REQUIRE(x && y && w && bias && scale && shift, "res2_dconv: null operand");
  F5E_REQUIRE(C > 0 && C % 8 == 0, "res2_dconv: C must be a positive multiple of 8 (got %d)", C);
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && ldx >= C && ldy >= C, "res2_dconv: need 0 < B <= 65535, T > 0, ldx / ldy >= C");
  F5E_REQUIRE(dilation >= 1 && dilation <= 64, "res2_dconv: dilation must be in [1, 64]");
  F5E_REQUIRE(first >= 0 && count >= 1 && first + count <= 7, "res2_dconv: steps [first, first + count) must lie in [0, 7)");
  F5E_REQUIRE(x != (const float*)y, "res2_dconv: in-place operation is not supported (neighbouring tiles read x)");
  Res2Args a{};
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy; a.w = w; a.bias = bias; a.scale = scale; a.shift = shift; a.len = len;
  a.T = T; a.wd = C / 8; a.d = dilation; a.first = first; a.count = count; a.copy_last = first + count == 7;
  const int wd = a.wd, wp = (wd + 3) & ~3, ocp = (wd + 15) & ~15;
  const int R = RES2_TT + 2 * count * dilation;
  const long long lds = 4ll * (2ll * R * (wp + 4) + (long long)ocp * (3 * wp + 4));
  F5E_REQUIRE(lds <= RES2_MAX_LDS, "res2_dconv: C = %d at dilation %d needs %lld B of LDS (limit %d)", C, dilation, lds,
              RES2_MAX_LDS);
  static F5eDeviceOnce lds_once;
  F5E_OPT_IN_LDS(lds_once, ecapa_res2_kernel, RES2_MAX_LDS);
  const dim3 grid((unsigned)((T + RES2_TT - 1) / RES2_TT), (unsigned)B);
  if (wd % 16 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && al16(x) && al16(y) && al16(w) && al16(bias) && al16(scale) && al16(shift)) {
    static F5eDeviceOnce lds_once_64, lds_once_w16;
    if (wd == 64) {
      F5E_OPT_IN_LDS(lds_once_64, ecapa_res2_w16_kernel<64>, RES2_MAX_LDS);
      hipLaunchKernelGGL(ecapa_res2_w16_kernel<64>, grid, dim3(RES2_NT), (size_t)lds, st, a);
    } else {
      F5E_OPT_IN_LDS(lds_once_w16, ecapa_res2_w16_kernel<0>, RES2_MAX_LDS);
      hipLaunchKernelGGL(ecapa_res2_w16_kernel<0>, grid, dim3(RES2_NT), (size_t)lds, st, a);
    }
  } else {
    hipLaunchKernelGGL(ecapa_res2_kernel, grid, dim3(256), (size_t)lds, st, a);
  }
  F5E_LAUNCH_CHECK("res2_dconv");
  return F5E_OK;
}

int f5e_time_stats(hipStream_t st, const float* x, int ldx, const int* len, float* mean, float* std_out, int ld_out, int B,
                   int T, int C) {
  F5E_REQUIRE(x && mean, "time_stats: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldx % 4 == 0 && ld_out >= C && ld_out % 4 == 0,
              "time_stats: need 0 < B <= 65535, T > 0, C / ldx / ld_out multiples of 4 with ldx, ld_out >= C");
  F5E_REQUIRE(al16(x) && al16(mean) && al16(std_out), "time_stats: operands must be 16-byte aligned");
  hipLaunchKernelGGL(ecapa_time_stats_kernel, dim3((unsigned)((C / 4 + 7) / 8), (unsigned)B), dim3(256), 0, st, x, ldx, len, mean,
                     std_out, ld_out, T, C / 4);
  F5E_LAUNCH_CHECK("time_stats");
  return F5E_OK;
}

int f5e_se_scale(hipStream_t st, const float* x, int ldx, const float* gate, const float* resid, int ldr, float* out, int ldo,
                 int B, int T, int C) {
  F5E_REQUIRE(x && gate && resid && out, "se_scale: null operand");
  F5E_REQUIRE(B > 0 && T > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldr >= C && ldo >= C && ldx % 4 == 0 && ldr % 4 == 0 &&
                  ldo % 4 == 0,
              "se_scale: need B, T > 0 and C / ldx / ldr / ldo multiples of 4 with every ld >= C");
  F5E_REQUIRE(al16(x) && al16(gate) && al16(resid) && al16(out), "se_scale: operands must be 16-byte aligned");
  const long long total = (long long)B * T * (C / 4);
  hipLaunchKernelGGL(ecapa_se_scale_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, ldx, gate, resid, ldr,
                     out, ldo, T, C / 4, total);
  F5E_LAUNCH_CHECK("se_scale");
  return F5E_OK;
}

int f5e_bias_tanh(hipStream_t st, float* x, int ldx, const float* add, int ld_add, int add_rows, int B, int T, int N) {
  F5E_REQUIRE(x && add, "bias_tanh: null operand");
  F5E_REQUIRE(B > 0 && T > 0 && N > 0 && ldx >= N && ld_add >= N && (add_rows == 1 || add_rows == B),
              "bias_tanh: need B, T, N > 0, ldx / ld_add >= N and add_rows 1 or B");
  const long long total = (long long)B * T * N;
  hipLaunchKernelGGL(ecapa_bias_tanh_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, x, ldx, add, ld_add,
                     add_rows, T, N, total);
  F5E_LAUNCH_CHECK("bias_tanh");
  return F5E_OK;
}

int f5e_attn_stats_pool(hipStream_t st, const float* x, int ldx, const float* logits, int ldl, const int* len, float* out,
                        int B, int T, int C) {
  F5E_REQUIRE(x && logits && out, "attn_stats_pool: null operand");
  F5E_REQUIRE(B > 0 && B <= 65535 && T > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldl >= C && ldx % 4 == 0 && ldl % 4 == 0,
              "attn_stats_pool: need 0 < B <= 65535, T > 0, C / ldx / ldl multiples of 4 with ldx, ldl >= C");
  F5E_REQUIRE(al16(x) && al16(logits) && al16(out), "attn_stats_pool: operands must be 16-byte aligned");
  hipLaunchKernelGGL(ecapa_pool_kernel, dim3((unsigned)((C / 4 + 7) / 8), (unsigned)B), dim3(256), 0, st, x, ldx, logits, ldl,
                     len, out, T, C / 4);
  F5E_LAUNCH_CHECK("attn_stats_pool");
  return F5E_OK;
}

}  // extern "C"
