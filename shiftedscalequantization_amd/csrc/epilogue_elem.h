// K13's forward element function, shared by the K13 forward (recon.hip, bias_act_kernel) and
// the kernels that apply the same epilogue inside another pass (actshift_epi.hip, K34).
#pragma once

#include "ssq_common.h"

namespace ssq {

// act(((v + bc) * gc + pc) + rv) in the reference's op order (conv bias add, gamma^z / phi^z,
// residual add, activation: one fp32 rounding each, no fma).  bias / AFFINE / RES say which of
// the operands exist: a missing one is skipped, not replaced by its identity (x + 0 and x * 1 + 0
// lose a -0).  The activation is torch's clamp: keeps -0 and NaN.
template <bool RES, int ACT, bool AFFINE>
__device__ __forceinline__ float k13_elem(bool bias, float v, float rv, float bc, float gc,
                                          float pc) {
  float t = bias ? __fadd_rn(v, bc) : v;
  if (AFFINE) t = __fadd_rn(__fmul_rn(t, gc), pc);  // out*alpha_out + beta_out
  if (RES) t = __fadd_rn(t, rv);
  return act_fwd<ACT>(t);
}

}  // namespace ssq
