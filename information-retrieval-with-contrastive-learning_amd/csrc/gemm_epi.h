// What the two bf16 GEMM translation units (gemm.hip, gemm_pp.hip) share on the device
// side: the epilogue codes, the GELU forms of the fp32-output epilogues, and the
// transposed LDS read.  One definition each, so a new epilogue or a change to the GELU
// polynomial reaches every kernel.
#pragma once
#include "irc_common.h"

namespace irc {
namespace gemm {

// Epilogue codes of irc_gemm (include/irc.h), plus the scan filter's internal one.
// EPI_DGELU: C = alpha acc * gelu'(R)  (GELU backward; R = saved pre-activation)
// EPI_BIAS_GELU_SAVE: C = gelu(alpha acc + bias) and R <- alpha acc + bias (R is a
// second OUTPUT here: the pre-activation the GELU backward needs)
// EPI_SCAN: the scan filter of gemm_pp.hip (see PArgs in gemm_pp.h); not an irc_gemm code
// EPI_PICK: the candidate pick of gemm_pp.hip (irc_rerank_topk_stream); not an irc_gemm code
// EPI_GROUP: the group maximum of gemm_pp.hip (irc_scan_topk_grouped); not an irc_gemm code
// EPI_PICK_BIAS: EPI_PICK with a per-candidate bias added to the score
// (irc_rerank_biased_topk); not an irc_gemm code
enum Epi {
  EPI_NONE = 0, EPI_BIAS = 1, EPI_BIAS_GELU = 2, EPI_BIAS_RESID = 3, EPI_RESID = 4,
  EPI_DGELU = 5, EPI_BIAS_GELU_SAVE = 6, EPI_SCAN = 7, EPI_PICK = 8, EPI_GROUP = 9,
  EPI_PICK_BIAS = 10
};
// Not constexpr on purpose: a predicate the front end can fold reshapes the bias preload's
// control flow in gemm_pp.hip, whose kernels sit at the 256-VGPR limit: all 57 of its
// epilogue 1 / 2 / 3 / 6 kernels change, and every such gemm_pp_pers_kernel spills more
// (scratch <true, true, *, 1|3|6> 0 -> 8 B/lane, <true, true, float, 2> 0 -> 20, the
// <true, false> ones 8 -> 12..24; -Rpass-analysis=kernel-resource-usage).  Inlined, it
// folds just the same later.
__host__ __device__ __forceinline__ bool epi_has_bias(int e) {
  return e == EPI_BIAS || e == EPI_BIAS_GELU || e == EPI_BIAS_RESID || e == EPI_BIAS_GELU_SAVE;
}

// ds_read_b64_tr_b16: hardware-transposed LDS read (a 16-lane group reads 4 k-rows x 16
// columns and each lane receives its column)
typedef short v4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4s ds_tr16(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4s*)(p));
}

// ---- GELU of the epilogues whose output stays fp32 (bf16 outputs: gelu_lite, irc_common.h)

// Library erf: the fp32 parity kernel (gemm_kernel).
__device__ __forceinline__ float gelu_erf(float x) {
  return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f));
}
__device__ __forceinline__ float gelu_grad_erf(float x) {
  return 0.5f * (1.0f + erff(x * 0.70710678118654752f)) +
         x * 0.3989422804014327f * __expf(-0.5f * x * x);
}

// GELU(x) = 0.5 x (1 + erf(x / sqrt 2)) with erf from Abramowitz & Stegun 7.1.26
// (|error| <= 1.5e-7 absolute, i.e. below fp32 resolution of the (1 + erf) sum
// for |x| >~ 1): ~15 branch-free VALU ops against the library erff's ~40, which
// matters when the epilogue is not hidden behind MFMA work (the big tiles).
__device__ __forceinline__ float gelu_fast(float x) {
  const float z = x * 0.70710678118654752f;
  const float az = fabsf(z);
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * az);
  float p = 1.061405429f;
  p = p * t - 1.453152027f;
  p = p * t + 1.421413741f;
  p = p * t - 0.284496736f;
  p = p * t + 0.254829592f;
  const float e = 1.0f - p * t * __expf(-az * az);
  return 0.5f * x * (1.0f + copysignf(e, z));
}
// d/dx GELU(x) = Phi(x) + x phi(x), Phi via the same A&S 7.1.26 erf as gelu_fast.
__device__ __forceinline__ float gelu_grad_fast(float x) {
  const float z = x * 0.70710678118654752f;
  const float az = fabsf(z);
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * az);
  float p = 1.061405429f;
  p = p * t - 1.453152027f;
  p = p * t + 1.421413741f;
  p = p * t - 0.284496736f;
  p = p * t + 0.254829592f;
  const float ez = __expf(-az * az);
  const float e = 1.0f - p * t * ez;
  return 0.5f * (1.0f + copysignf(e, z)) + x * 0.3989422804014327f * ez;
}

// Two lanes' worth of gelu_fast / gelu_grad_fast on <2 x float>: the polynomial, scale
// and blend steps issue as v_pk_fma_f32 / v_pk_mul_f32 (2 results per lane per op), only
// rcp / exp / copysign stay scalar.  The same operations in the same order as the scalar
// forms.  The epilogue of the 256x256 tile is VALU-bound (one workgroup per CU, nothing
// to overlap it with), so this is the FFN1 + GELU launch's tail.
__device__ __forceinline__ void erf_as_parts(f32x2_t x, f32x2_t& z, f32x2_t& t, f32x2_t& ez) {
  z = x * 0.70710678118654752f;
  f32x2_t az = {fabsf(z.x), fabsf(z.y)};
  const f32x2_t d = 1.0f + 0.3275911f * az;
  t = f32x2_t{__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
  const f32x2_t n = -az * az;
  ez = f32x2_t{__expf(n.x), __expf(n.y)};
}
__device__ __forceinline__ f32x2_t erf_as_poly(f32x2_t t) {
  f32x2_t p = 1.061405429f * t - 1.453152027f;
  p = p * t + 1.421413741f;
  p = p * t - 0.284496736f;
  p = p * t + 0.254829592f;
  return p;
}
__device__ __forceinline__ f32x2_t gelu_f2(f32x2_t x) {
  f32x2_t z, t, ez;
  erf_as_parts(x, z, t, ez);
  const f32x2_t e = 1.0f - erf_as_poly(t) * t * ez;
  const f32x2_t s = {copysignf(e.x, z.x), copysignf(e.y, z.y)};
  return 0.5f * x * (1.0f + s);
}
__device__ __forceinline__ f32x2_t gelu_grad_f2(f32x2_t x) {
  f32x2_t z, t, ez;
  erf_as_parts(x, z, t, ez);
  const f32x2_t e = 1.0f - erf_as_poly(t) * t * ez;
  const f32x2_t s = {copysignf(e.x, z.x), copysignf(e.y, z.y)};
  return 0.5f * (1.0f + s) + x * 0.3989422804014327f * ez;
}

}  // namespace gemm
}  // namespace irc
