// Device-side pieces the optimizer kernels share (optim.hip: Adam, lamb.hip: LAMB): the by-value group
// table of an eager step and the model EMA of the update pass.
#pragma once
#include "common.h"
#include "kernels.h"

namespace pvr {

// Group table (AdamGroup rows: kernels.h) passed by value in the kernel arguments (eager stepping: no per-step host-to-device
// copy); graph-captured steps pass a device table instead (kernel arguments are frozen at capture).
constexpr int MAX_ARG_GROUPS = 8;
struct AdamGroupArgs {
  AdamGroup g[MAX_ARG_GROUPS];
};

// Model EMA inside the Adam pass (AdamEma: kernels.h). The kernels are templates on EMA: the default
// instantiation takes an empty argument and is the instruction stream it was without the feature; the
// EMA one reads and writes one more fp32 buffer with the layout of p,
//   ema = decay * ema + one_minus_decay * p_new
// for exactly the elements Adam updates (frozen segments and a skipped non-finite step leave it alone).
// Two products, not ema + w * (p - ema): decay 0 gives p_new and decay 1 leaves ema, bit for bit,
// contracted to an fma or not.
template <bool EMA> struct EmaArg {};
template <> struct EmaArg<true> { AdamEma a; };

namespace {

// {decay, one_minus_decay} of this launch: the device pair (graph-captured steps) or the by-value one
__device__ __forceinline__ float2 ema_pair(const AdamEma& a) {
  return a.pair ? make_float2(a.pair[0], a.pair[1]) : make_float2(a.decay, a.one_minus_decay);
}

// Every call sits behind a test of the buffer pointer (which the host never leaves null), after the
// Adam update of the values it reads: a branch of its own keeps the EMA's arithmetic out of the basic
// block of the Adam update. In one block the vectoriser pairs operations across the two and changes
// which of Adam's a * b + c are contracted, so the EMA instantiation rounded p, m and v differently from
// the default one (tests/test_gpu_model_ema.py compares the two bit for bit). The branch is uniform.
__device__ __forceinline__ void ema4(float* __restrict__ ema, int64_t e, const float4& pp, float2 dw) {
  float4 ee = *(float4*)(ema + e);
  ee.x = dw.x * ee.x + dw.y * pp.x;
  ee.y = dw.x * ee.y + dw.y * pp.y;
  ee.z = dw.x * ee.z + dw.y * pp.z;
  ee.w = dw.x * ee.w + dw.y * pp.w;
  *(float4*)(ema + e) = ee;
}

// host: copy a [ngroups] table into the by-value kernel argument (false: too many groups)
inline bool adam_group_args(const AdamGroup* host, int ngroups, AdamGroupArgs& out) {
  if (!host || ngroups <= 0 || ngroups > MAX_ARG_GROUPS) return false;
  for (int i = 0; i < ngroups; ++i) out.g[i] = host[i];
  return true;
}

}  // namespace
}  // namespace pvr
