// f5e_gemm_f32_skinny: out[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) + addend[m][n] for 1 <= M <= 16 rows, fp32.
//
// A handful of rows against a weight matrix is a read of W and nothing else, so the launch exists to stream W ONCE at a rate
// that involves the whole chip.  f5e_gemm_f32's 32 x 64 tiles give 20 workgroups at N = 1280: here W is cut into tiles of 16
// rows, and where that leaves fewer than two workgroups per CU also along K.
//
//   * a wave owns 16 rows of W and a range of 16-float chunks of K.  Lane (c16, g) loads the float4 W[n0 + c16][16 c + 4 g ..]
//     (a row of the tile is read 64 contiguous bytes at a time, four chunks in flight per lane) and the float4 A[c16][same k];
//     four v_mfma_f32_16x16x4_f32 per chunk leave out[4 g + i][n0 + c16] in the lane.  Rows of A at or beyond M repeat row
//     M - 1 and are never stored, so a row's result does not depend on M.
//   * the four waves of a workgroup take consecutive K ranges of one tile and are summed through LDS in wave order;
//   * with KS > 1 K-slices per tile (N small), slice s writes its partial tile to workspace[s][m][n] and a second launch sums
//     the slices in order s = 0 .. KS - 1 and applies bias, activation and addend.  KS is a function of N, K and the CU count
//     alone.  No floating-point atomics: a launch is bit-reproducible.
//   * addend may alias out: each element is read once and written by the same lane.
#include "f5e_common.h"
#include "gemm_f32_skinny_body.h"   // the kernels: one body for this file and gemm_f32_w16.hip

int f5e_gemm_f32_skinny_workspace(int N, int K, unsigned long long* bytes_out_host) {
  return skinny_workspace("gemm_f32_skinny_workspace", N, K, bytes_out_host);
}

int f5e_gemm_f32_skinny(hipStream_t st, const float* A, int lda, const float* W, int ldw, const float* bias, int act,
                        const float* addend, int ld_add, float* out, int ldo, void* workspace, unsigned long long workspace_bytes,
                        int M, int N, int K) {
  return skinny_launch<WLoadF32, 4>("gemm_f32_skinny", st, A, lda, W, ldw, 16, bias, act, addend, ld_add, out, ldo, workspace,
                                    workspace_bytes, M, N, K);
}
