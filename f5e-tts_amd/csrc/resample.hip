// Polyphase windowed-sinc sample-rate conversion for any rational ratio orig : new (the arithmetic of
// infer/audio.py::resample, which restates torchaudio's sinc_interp_hann):
//   y[b][f * new + p] = sum_k bank[p][k] * x[b][f * orig + k - width],   0 <= k < taps = 2 * width + orig,
// x read as 0 outside [0, n).  Replaces the host F.conv1d (and the D2H / H2D copies either side of it) in front of the mel
// and kaldi-fbank kernels of the voice-conversion path.
//
// A workgroup owns FR consecutive frames x PH consecutive phases of one row:
//   * the input window of those frames ((FR - 1) * orig + taps samples) is staged into LDS once; every phase of a frame
//     reads the same window, and consecutive frames overlap by taps - orig samples;
//   * the PH bank rows are staged TRANSPOSED, bt[k][PHP]: lanes that differ in phase then read consecutive words (no bank
//     conflict whatever `taps` is), lanes that share a phase read one word (broadcast).  PHP = PH | 1 keeps the staging
//     writes (stride PHP words, lanes along k) off a common bank as well;
//   * lanes run along the output index (phase fastest), so a wave's stores are contiguous runs of PH floats.
// The bank can be larger than LDS (441 : 160 with 475 taps is 304 KB): PH is then the largest phase count whose rows fit
// the 32 KiB bank share, and blockIdx.y walks the phase subsets.  A bank that fits (3 : 2 is 2 x 23) is one subset: one
// workgroup column, fully contiguous stores, no second pass over x.
// Each output is a taps-term dot product in eight interleaved fp32 FMA chains (k mod 8) combined pairwise: rounding grows
// with taps / 8, like the vector accumulators of the host convolution, not with taps.
// No allocation, no synchronisation; nothing is written past n_out in a row or into the gap ld_y - n_out.
#include "f5e_common.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_BANK_FLOATS = 8192;  // 32 KiB: transposed bank rows of one phase subset
constexpr int RS_X_FLOATS = 8192;     // 32 KiB: input window of one frame tile
constexpr int RS_TARGET = 512;        // outputs per workgroup aimed at (two per thread)

__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, long long ld_x,
                                                              const float* __restrict__ bank, float* __restrict__ y,
                                                              long long ld_y, int orig, int nw, int width, int taps, int n,
                                                              int n_out, int n_frames, int FR, int PH, int PHP) {
  extern __shared__ float lds[];
  float* bt = lds;               // [taps][PHP]
  float* xs = lds + taps * PHP;  // [(fr - 1) * orig + taps]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int f0 = blockIdx.x * FR, p0 = blockIdx.y * PH;
  const int fr = min(FR, n_frames - f0), ph = min(PH, nw - p0);

  for (int pl = wave; pl < ph; pl += RS_THREADS / 64) {
    const float* row = bank + (long long)(p0 + pl) * taps;
    for (int k = lane; k < taps; k += 64) bt[k * PHP + pl] = row[k];
  }
  const int span = (fr - 1) * orig + taps;
  const long long g0 = (long long)f0 * orig - width;
  const float* xr = x + (long long)blockIdx.z * ld_x;
  for (int j = tid; j < span; j += RS_THREADS) {
    const long long g = g0 + j;
    xs[j] = (g >= 0 && g < n) ? xr[g] : 0.f;
  }
  __syncthreads();

  float* yr = y + (long long)blockIdx.z * ld_y;
  for (int i = tid; i < fr * ph; i += RS_THREADS) {
    const int fl = i / ph, pl = i - fl * ph;
    const long long o = (long long)(f0 + fl) * nw + p0 + pl;
    if (o >= n_out) continue;  // the last frame may be partial
    const float* xp = xs + fl * orig;
    const float* bp = bt + pl;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int k = 0;
    for (; k + 8 <= taps; k += 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = __builtin_fmaf(bp[(k + j) * PHP], xp[k + j], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j)
      if (k + j < taps) acc[j] = __builtin_fmaf(bp[(k + j) * PHP], xp[k + j], acc[j]);
    yr[o] = ((acc[0] + acc[4]) + (acc[2] + acc[6])) + ((acc[1] + acc[5]) + (acc[3] + acc[7]));
  }
}

}  // namespace

int f5e_resample(hipStream_t st, const float* x, long long ld_x, const float* bank, int orig, int nw, int width, float* y,
                 long long ld_y, int B, int n, int n_out) {
  F5E_REQUIRE(x && bank && y, "resample: null operand");
  F5E_REQUIRE(orig >= 1 && nw >= 1 && width >= 0 && n >= 1 && B >= 1 && B <= 65535,
              "resample: need orig, new, n >= 1, width >= 0 and 1 <= B <= 65535 (orig %d new %d width %d n %d B %d)", orig, nw,
              width, n, B);
  const long long want = ((long long)nw * n + orig - 1) / orig;
  F5E_REQUIRE(want <= 0x7fffffffLL && n_out == (int)want, "resample: n_out %d, ceil(new * n / orig) = %lld", n_out, want);
  F5E_REQUIRE(ld_x >= n && ld_y >= n_out, "resample: row stride smaller than the row (ld_x %lld < %d or ld_y %lld < %d)", ld_x,
              n, ld_y, n_out);
  const long long taps_ll = 2ll * width + orig;
  if (taps_ll > RS_BANK_FLOATS / 2) {  // one phase row (and one frame's window) must fit its LDS share with room to tile
    f5e_set_error("resample: %lld taps (ratio %d : %d) exceed the kernel's %d", taps_ll, orig, nw, RS_BANK_FLOATS / 2);
    return F5E_ERR_UNSUPPORTED;
  }
  const int taps = (int)taps_ll;
  // phases per workgroup: all of them when the bank fits, else the largest subset whose padded rows do
  int PH = nw;
  if ((long long)(nw | 1) * taps > RS_BANK_FLOATS) {
    PH = RS_BANK_FLOATS / taps;
    if (!(PH & 1) && (PH | 1) * taps > RS_BANK_FLOATS) PH -= 1;
  }
  const int PHP = PH | 1;
  const int n_frames = (n_out + nw - 1) / nw;
  int FR = (RS_TARGET + PH - 1) / PH;
  FR = min(FR, (RS_X_FLOATS - taps) / orig + 1);
  FR = max(1, min(FR, n_frames));
  const long long tiles = ((long long)n_frames + FR - 1) / FR;
  const int ptiles = (nw + PH - 1) / PH;
  F5E_REQUIRE(tiles <= 0x7fffffffLL && ptiles <= 65535, "resample: grid %lld x %d too large", tiles, ptiles);
  const size_t lds = ((size_t)taps * PHP + (size_t)(FR - 1) * orig + taps) * sizeof(float);  // <= 64 KiB by construction
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)tiles, (unsigned)ptiles, (unsigned)B), dim3(RS_THREADS), lds, st, x, ld_x,
                     bank, y, ld_y, orig, nw, width, taps, n, n_out, n_frames, FR, PH, PHP);
  F5E_LAUNCH_CHECK("resample");
  return F5E_OK;
}
