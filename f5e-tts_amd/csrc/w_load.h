// How a kernel of the fp32 GEMM family reads four consecutive elements of its weight operand: as they are (fp32), or 16-bit
// and widened in registers (gemm_f32_w16.hip, DESIGN 4o "16-bit weights").  Widening is exact, so the MFMA behind the load
// sees the operand values of the fp32 path on the widened copy of W, and the bits of the result are that path's.
//   bf16: the 16 bits are the high half of the float;
//   fp16: v_cvt_f32_f16 (subnormals are kept: the kernels run with fp16 / fp64 denormals enabled, hipcc's default).
#pragma once
#include "f5e_common.h"

typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

struct WLoadF32 {
  typedef float elem;
  static __device__ __forceinline__ f32x4 load4(const float* p) { return *(const f32x4*)p; }
  static __device__ __forceinline__ f32x4 load4_stream(const float* p) { return __builtin_nontemporal_load((const f32x4*)p); }
};

template <int WTYPE>   // F5E_W_FP16 or F5E_W_BF16
struct WLoad16 {
  typedef unsigned short elem;
  static __device__ __forceinline__ f32x4 widen(u32x2 raw) {
    if constexpr (WTYPE == F5E_W_BF16)
      return f32x4{__uint_as_float(raw[0] << 16), __uint_as_float(raw[0] & 0xffff0000u), __uint_as_float(raw[1] << 16),
                   __uint_as_float(raw[1] & 0xffff0000u)};
    else
      return __builtin_convertvector(__builtin_bit_cast(f16x4, raw), f32x4);
  }
  static __device__ __forceinline__ f32x4 load4(const elem* p) { return widen(*(const u32x2*)p); }
  static __device__ __forceinline__ f32x4 load4_stream(const elem* p) { return widen(__builtin_nontemporal_load((const u32x2*)p)); }
};
