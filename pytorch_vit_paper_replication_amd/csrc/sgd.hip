// SGD with momentum over the flat parameter store: torch.optim.SGD (dampening 0) as one pass behind the
// two norm launches of optim.hip, in the two forms the Adam pass has (optim.hip adam_kernel / adam_t_kernel):
// the segment-table form and the tile form that also writes the transposed bf16 shadow W^T of the
// registered 2-D weights. One fp32 state buffer instead of Adam's two: a 2-D weight moves 24 bytes per
// element (p, g, buf read; p, buf, shadow, W^T written) against 32.
// Group rows are AdamGroup rows (kernels.h): lr, beta1 as the momentum, weight_decay, SGD_NESTEROV in word 7.
#include "common.h"
#include "kernels.h"
#include "optim_device.h"

namespace pvr {

namespace {

constexpr int SGD_BLOCKS = 8192;       // grid cap of the segment-table form
constexpr int SGD_FLAT_BLOCKS = 1024;  // grid-stride blocks of the tile form's flat ranges

// What a group's row says, decoded once per float4 (per tile in the tile blocks)
struct SgdRow {
  float neg_lr, mom, wd;
  bool nesterov;
};
__device__ __forceinline__ SgdRow sgd_row(const AdamGroup& G) {
  return SgdRow{-G.lr, G.beta1, G.weight_decay, (G.decoupled & SGD_NESTEROV) != 0};
}

// Every a * b + c of the update is an explicit fma, so the rounding does not depend on what the compiler
// contracts in one instantiation or another: the two forms and their EMA variants give the same bits.
// g' of the formula; wd is uniform over the segment
__device__ __forceinline__ float4 sgd_grad4(const float4& pp, const float4& gg, const SgdRow& r, float gscale) {
  float4 gr = make_float4(gg.x * gscale, gg.y * gscale, gg.z * gscale, gg.w * gscale);
  if (r.wd != 0.f) {
    gr.x = __fmaf_rn(r.wd, pp.x, gr.x); gr.y = __fmaf_rn(r.wd, pp.y, gr.y);
    gr.z = __fmaf_rn(r.wd, pp.z, gr.z); gr.w = __fmaf_rn(r.wd, pp.w, gr.w);
  }
  return gr;
}
// buf = mom * buf + g', and the direction d (Nesterov: g' + mom * buf)
__device__ __forceinline__ float4 sgd_momentum4(float4& bb, const float4& gr, const SgdRow& r) {
  bb.x = __fmaf_rn(r.mom, bb.x, gr.x); bb.y = __fmaf_rn(r.mom, bb.y, gr.y);
  bb.z = __fmaf_rn(r.mom, bb.z, gr.z); bb.w = __fmaf_rn(r.mom, bb.w, gr.w);
  if (!r.nesterov) return bb;
  return make_float4(__fmaf_rn(r.mom, bb.x, gr.x), __fmaf_rn(r.mom, bb.y, gr.y), __fmaf_rn(r.mom, bb.z, gr.z),
                     __fmaf_rn(r.mom, bb.w, gr.w));
}
__device__ __forceinline__ void sgd_apply4(float4& pp, const float4& d, const SgdRow& r) {
  pp.x = __fmaf_rn(r.neg_lr, d.x, pp.x); pp.y = __fmaf_rn(r.neg_lr, d.y, pp.y);
  pp.z = __fmaf_rn(r.neg_lr, d.z, pp.z); pp.w = __fmaf_rn(r.neg_lr, d.w, pp.w);
}

// One float4 at flat element e: p and, where the group has momentum, buf updated in memory; returns the
// new p. buf of a group without momentum is neither read nor written (the branch is segment-uniform).
__device__ __forceinline__ float4 sgd_update4(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t e,
                                              const SgdRow& r, float gscale) {
  float4 pp = *(float4*)(p + e);
  const float4 gg = *(const float4*)(g + e);
  const float4 gr = sgd_grad4(pp, gg, r, gscale);
  if (r.mom != 0.f) {
    float4 bb = *(float4*)(buf + e);
    const float4 d = sgd_momentum4(bb, gr, r);
    *(float4*)(buf + e) = bb;
    sgd_apply4(pp, d, r);
  } else {
    sgd_apply4(pp, gr, r);
  }
  *(float4*)(p + e) = pp;
  return pp;
}

// seg_start[i] = first flat index of segment i (sorted, multiples of 4, seg_start[0] = 0), seg_group[i] its
// param group (-1: frozen / padding): the tables of adam_kernel.
template <bool EMA>
__global__ void __launch_bounds__(256) sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                   uint16_t* __restrict__ shadow, int64_t n, const int64_t* __restrict__ seg_start,
                                                   const int* __restrict__ seg_group, int nseg, const AdamGroup* __restrict__ groups,
                                                   AdamGroupArgs garg, const float* __restrict__ clip, int skip_nonfinite,
                                                   EmaArg<EMA> ea) {
  const float gscale = clip ? clip[1] : 1.f;
  if (clip && skip_nonfinite && clip[2] != 0.f) return;
  float2 dw = make_float2(0.f, 0.f);
  if constexpr (EMA) dw = ema_pair(ea.a);
  const int64_t n4 = n / 4;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t e = i * 4;
    int lo = 0, hi = nseg - 1;  // the segment containing e
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (seg_start[mid] <= e) lo = mid; else hi = mid - 1;
    }
    const int gi = seg_group[lo];
    if (gi < 0) continue;  // frozen / padding
    const SgdRow r = sgd_row(groups ? groups[gi] : garg.g[gi]);
    const float4 pp = sgd_update4(p, g, buf, e, r, gscale);
    if constexpr (EMA) {
      if (ea.a.buf != nullptr) ema4(ea.a.buf, e, pp, dw);
    }
    if (shadow) *(uint2*)(shadow + e) = make_uint2(pack2bf(pp.x, pp.y), pack2bf(pp.z, pp.w));
  }
}

// The tile form, with adam_t_kernel's tables and block roles. Blocks [0, ntiles): one 64x64 fp32 tile of a
// registered 2-D weight W [R][C]; p / g / buf row-major (16 lanes x 16 B per 256-B row), the bf16 values to
// the shadow and, through a [64][33] x 2-bf16 LDS image, to W^T [C][R] as 16-B pieces. Blocks [ntiles, grid):
// grid-stride over the flat ranges of fmeta.
template <bool EMA>
__global__ void __launch_bounds__(256) sgd_t_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                     uint16_t* __restrict__ shadow, uint16_t* __restrict__ shadow_t,
                                                     const int64_t* __restrict__ tmeta, int nmat, int ntiles,
                                                     const int64_t* __restrict__ fmeta, int nflat, int64_t flat4,
                                                     const AdamGroup* __restrict__ groups, AdamGroupArgs garg,
                                                     const float* __restrict__ clip, int skip_nonfinite, EmaArg<EMA> ea) {
  const float gscale = clip ? clip[1] : 1.f;
  if (clip && skip_nonfinite && clip[2] != 0.f) return;
  float2 dw = make_float2(0.f, 0.f);
  if constexpr (EMA) dw = ema_pair(ea.a);
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < ntiles) {
    __shared__ uint32_t tile[64][33];
    const int blk = blockIdx.x;
    int lo = 0, hi = nmat - 1;  // last weight whose first tile <= blk
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tmeta[mid * 6 + 4] <= blk) lo = mid; else hi = mid - 1;
    }
    const int64_t soff = tmeta[lo * 6 + 0], doff = tmeta[lo * 6 + 1];
    const int R = (int)tmeta[lo * 6 + 2], C = (int)tmeta[lo * 6 + 3];
    const int gi = (int)tmeta[lo * 6 + 5];
    const int local = blk - (int)tmeta[lo * 6 + 4];
    const int tc = C / 64;
    const int r0 = (local / tc) * 64, c0 = (local % tc) * 64;
    if (gi < 0) return;  // frozen: master, shadow and W^T unchanged
    const SgdRow r = sgd_row(groups ? groups[gi] : garg.g[gi]);
    const int cq = (tid & 15) * 4;
    const int64_t e0 = soff + (int64_t)(r0 + (tid >> 4)) * C + c0 + cq;  // row (tid >> 4) + 16 it is 16 C further
    // all twelve (eight without momentum) loads of the thread are issued before the first dependent use
    float4 pp[4], gg[4], bb[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      pp[it] = *(float4*)(p + e0 + (int64_t)it * 16 * C);
      gg[it] = *(const float4*)(g + e0 + (int64_t)it * 16 * C);
    }
    if (r.mom != 0.f) {
#pragma unroll
      for (int it = 0; it < 4; ++it) bb[it] = *(float4*)(buf + e0 + (int64_t)it * 16 * C);
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const float4 gr = sgd_grad4(pp[it], gg[it], r, gscale);
        const float4 d = sgd_momentum4(bb[it], gr, r);
        *(float4*)(buf + e0 + (int64_t)it * 16 * C) = bb[it];
        sgd_apply4(pp[it], d, r);
      }
    } else {
#pragma unroll
      for (int it = 0; it < 4; ++it) sgd_apply4(pp[it], sgd_grad4(pp[it], gg[it], r, gscale), r);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = (tid >> 4) + 16 * it;
      const int64_t e = e0 + (int64_t)it * 16 * C;
      *(float4*)(p + e) = pp[it];
      const uint32_t lo2 = pack2bf(pp[it].x, pp[it].y), hi2 = pack2bf(pp[it].z, pp[it].w);
      *(uint2*)(shadow + e) = make_uint2(lo2, hi2);
      tile[row][cq >> 1] = lo2;
      tile[row][(cq >> 1) + 1] = hi2;
    }
    if constexpr (EMA) {
      if (ea.a.buf != nullptr) {
#pragma unroll
        for (int it = 0; it < 4; ++it) ema4(ea.a.buf, e0 + (int64_t)it * 16 * C, pp[it], dw);
      }
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + 256 * it;
      const int cc = idx / 8, rch = idx % 8;  // W^T row c0 + cc, W rows r0 + 8 rch .. + 7
      uint32_t h[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = (tile[rch * 8 + j][cc >> 1] >> ((cc & 1) * 16)) & 0xFFFFu;
      uint4 o;
      o.x = h[0] | (h[1] << 16); o.y = h[2] | (h[3] << 16); o.z = h[4] | (h[5] << 16); o.w = h[6] | (h[7] << 16);
      *(uint4*)(shadow_t + doff + (int64_t)(c0 + cc) * R + r0 + rch * 8) = o;
    }
    return;
  }
  const int64_t nblk = (int64_t)gridDim.x - ntiles;
  for (int64_t i = ((int64_t)blockIdx.x - ntiles) * 256 + tid; i < flat4; i += nblk * 256) {
    int lo = 0, hi = nflat - 1;  // range holding float4 i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (fmeta[mid * 4 + 3] <= i) lo = mid; else hi = mid - 1;
    }
    const int gi = (int)fmeta[lo * 4 + 2];
    if (gi < 0) continue;
    const int64_t e = fmeta[lo * 4 + 0] + (i - fmeta[lo * 4 + 3]) * 4;
    const SgdRow r = sgd_row(groups ? groups[gi] : garg.g[gi]);
    const float4 pp = sgd_update4(p, g, buf, e, r, gscale);
    *(uint2*)(shadow + e) = make_uint2(pack2bf(pp.x, pp.y), pack2bf(pp.z, pp.w));
    if constexpr (EMA) {
      if (ea.a.buf != nullptr) ema4(ea.a.buf, e, pp, dw);
    }
  }
}

}  // namespace
}  // namespace pvr

extern "C" int pvr_sgd_blocks() { return pvr::SGD_BLOCKS; }

extern "C" hipError_t pvr_sgd(float* p, const float* g, float* buf, uint16_t* shadow, int64_t n, const int64_t* seg_start,
                              const int* seg_group, int nseg, const pvr::AdamGroup* groups, const pvr::AdamGroup* host_groups,
                              int ngroups, const float* clip, int skip_nonfinite, pvr::AdamEma ema, hipStream_t s) {
  using namespace pvr;
  if (n <= 0) return hipSuccess;
  if (n % 4 != 0 || nseg <= 0) return hipErrorInvalidValue;
  AdamGroupArgs ga{};
  if (!groups && !adam_group_args(host_groups, ngroups, ga)) return hipErrorInvalidValue;
  int64_t blocks = (n / 4 + 255) / 256;
  if (blocks > SGD_BLOCKS) blocks = SGD_BLOCKS;
  if (ema.buf) {
    hipLaunchKernelGGL(sgd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, p, g, buf, shadow, n, seg_start, seg_group, nseg,
                       groups, ga, clip, skip_nonfinite, EmaArg<true>{ema});
  } else {
    hipLaunchKernelGGL(sgd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, p, g, buf, shadow, n, seg_start, seg_group, nseg,
                       groups, ga, clip, skip_nonfinite, EmaArg<false>{});
  }
  return hipGetLastError();
}

extern "C" hipError_t pvr_sgd_t(float* p, const float* g, float* buf, uint16_t* shadow, uint16_t* shadow_t, const int64_t* tmeta,
                                int nmat, int ntiles, const int64_t* fmeta, int nflat, int64_t flat4, const pvr::AdamGroup* groups,
                                const pvr::AdamGroup* host_groups, int ngroups, const float* clip, int skip_nonfinite,
                                pvr::AdamEma ema, hipStream_t s) {
  using namespace pvr;
  if (nmat <= 0 || ntiles <= 0 || nflat <= 0) return hipErrorInvalidValue;
  AdamGroupArgs ga{};
  if (!groups && !adam_group_args(host_groups, ngroups, ga)) return hipErrorInvalidValue;
  int64_t fb = (flat4 + 255) / 256;
  if (fb > SGD_FLAT_BLOCKS) fb = SGD_FLAT_BLOCKS;
  if (fb < 1) fb = 1;
  if (ema.buf) {
    hipLaunchKernelGGL(sgd_t_kernel<true>, dim3((unsigned)(ntiles + fb)), dim3(256), 0, s, p, g, buf, shadow, shadow_t, tmeta, nmat,
                       ntiles, fmeta, nflat, flat4, groups, ga, clip, skip_nonfinite, EmaArg<true>{ema});
  } else {
    hipLaunchKernelGGL(sgd_t_kernel<false>, dim3((unsigned)(ntiles + fb)), dim3(256), 0, s, p, g, buf, shadow, shadow_t, tmeta, nmat,
                       ntiles, fmeta, nflat, flat4, groups, ga, clip, skip_nonfinite, EmaArg<false>{});
  }
  return hipGetLastError();
}
