// The fp32 GEMMs with a 16-bit weight operand ("16-bit weights"): W is fp16 or bf16, row-major [N][ldw] (ldw in
// elements), and is widened to fp32 IN REGISTERS on its way from global memory (w_load.h).  Activations, accumulation, bias,
// epilogue and outputs stay fp32.  Widening is exact, the kernels are the fp32 kernels' own bodies with another loader
// (gemm_f32_tile.h, gemm_f32_skinny_body.h), and so every MFMA sees the operand values, in the slots and in the order, that
// the fp32 entry point gives it on the widened copy of W: the results are bit-equal, at half the bytes of W.
//
//   f5e_gemm_f32_w16_skinny   f5e_gemm_f32_skinny for 1 <= M <= 16: the decode step's launch, which is a read of W and nothing
//                             else.  A lane's load per chunk is 8 bytes here (the element-to-MFMA assignment is the fp32
//                             kernel's, so four elements of a chunk are all a lane may take), so it keeps 8 chunks in flight
//                             where the fp32 kernel keeps 4: the same 64 bytes of W and twice the bytes of A per lane.
//   f5e_gemm_f32_w16          f5e_gemm_f32 above 16 rows: the register-staged 64 x 64 tile.  f5e_gemm_f32 hands 16-byte aligned
//                             operands without an A-side activation to its LDS-DMA kernel, which cannot widen; this file runs
//                             the tile with that kernel's k-to-slot order instead (DMA_ORDER), and gives its bits.
#include "f5e_common.h"
#include "gemm_f32_skinny_body.h"
#include "gemm_f32_tile.h"

#define F5E_W16_REQUIRE(name)                                                                                          \
  F5E_REQUIRE(wtype == F5E_W_FP16 || wtype == F5E_W_BF16, name ": wtype %d is neither F5E_W_FP16 nor F5E_W_BF16", wtype)

int f5e_gemm_f32_w16_skinny_workspace(int N, int K, unsigned long long* bytes_out_host) {
  return skinny_workspace("gemm_f32_w16_skinny_workspace", N, K, bytes_out_host);
}

int f5e_gemm_f32_w16_skinny(hipStream_t st, const float* A, int lda, const void* W, int ldw, int wtype, const float* bias, int act,
                            const float* addend, int ld_add, float* out, int ldo, void* workspace,
                            unsigned long long workspace_bytes, int M, int N, int K) {
  F5E_W16_REQUIRE("gemm_f32_w16_skinny");
  if (wtype == F5E_W_FP16)
    return skinny_launch<WLoad16<F5E_W_FP16>, 8>("gemm_f32_w16_skinny", st, A, lda, W, ldw, 8, bias, act, addend, ld_add, out, ldo,
                                                 workspace, workspace_bytes, M, N, K);
  return skinny_launch<WLoad16<F5E_W_BF16>, 8>("gemm_f32_w16_skinny", st, A, lda, W, ldw, 8, bias, act, addend, ld_add, out, ldo,
                                               workspace, workspace_bytes, M, N, K);
}

int f5e_gemm_f32_w16(hipStream_t st, const float* A, int lda, int a_rows, int a_act, const void* W, int ldw, int wtype,
                     const float* bias, int act, const float* ch_scale, const float* addend, int ld_add, int add_rows,
                     const float* row_scale, float* out, int ldo, void* out_bf16, int ldo_bf16, int M, int N, int K) {
  F5E_W16_REQUIRE("gemm_f32_w16");
  Gemm32Args a;
  const int rc = gemm32_args("gemm_f32_w16", a, A, lda, a_rows, a_act, W, ldw, bias, act, ch_scale, addend, ld_add, add_rows,
                             row_scale, out, ldo, out_bf16, ldo_bf16, M, N, K);
  if (rc != F5E_OK) return rc;
  F5E_REQUIRE(((uintptr_t)W & 7) == 0, "gemm_f32_w16: W must be 8-byte aligned");
  // the widened copy this launch stands for is taken as 16-byte aligned (any allocation of its own is)
  const bool dma_order = gemm32_dma_order(a_act, A, nullptr);
  if (wtype == F5E_W_FP16)
    return dma_order ? gemm32_launch_tile<WLoad16<F5E_W_FP16>, true>("gemm_f32_w16", a, st)
                     : gemm32_launch_tile<WLoad16<F5E_W_FP16>, false>("gemm_f32_w16", a, st);
  return dma_order ? gemm32_launch_tile<WLoad16<F5E_W_BF16>, true>("gemm_f32_w16", a, st)
                   : gemm32_launch_tile<WLoad16<F5E_W_BF16>, false>("gemm_f32_w16", a, st);
}
