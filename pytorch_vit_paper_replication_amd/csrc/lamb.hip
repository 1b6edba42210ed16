// LAMB (You et al. 2019) over the flat parameter store: Adam's update, rescaled per parameter tensor by
// the trust ratio ||w|| / ||u||. Three launches behind the grad_norm pair of optim.hip:
//   1. lamb_moments_kernel  g * coef -> m, v; per 4096-element chunk of a tensor {sum p^2, sum u^2}
//   2. lamb_ratio_kernel    per tensor: the chunk sums in double -> trust = {||w||, ||u||, r}
//   3. lamb_update_kernel   u again from the new m, v -> p -= lr * r * u -> bf16 shadow, W^T, model EMA
// u is computed twice and never stored: both ways move 24 + 20 bytes per element, and a buffer for u
// would cost 4 bytes per parameter. No atomics, every sum in a fixed order: a step is bitwise repeatable.
#include "common.h"
#include "kernels.h"
#include "optim_device.h"

namespace pvr {
namespace {

// u of one element from its new moments. The weight-decay term is an explicit fma, so launches 1 and 3
// round it alike whatever the compiler contracts around it. Padding (p = m = v = 0) gives 0 / eps = 0.
__device__ __forceinline__ float lamb_u(float p, float m, float v, const AdamGroup& G) {
  const float a = (m / G.bc1) / (sqrtf(v) / G.bc2_sqrt + G.eps);
  return G.weight_decay != 0.f ? __fmaf_rn(G.weight_decay, p, a) : a;
}

__device__ __forceinline__ bool lamb_adapts(const AdamGroup& G) {
  return G.weight_decay != 0.f || (G.decoupled & LAMB_ALWAYS_ADAPT) != 0;
}

// One workgroup per chunk. Thread t takes float4 t, t + 256, t + 512, t + 768 of the chunk and adds its
// (at most 16) squares in that order; then the wave's butterfly, then the four waves in a fixed order.
__global__ void __launch_bounds__(256) lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                           const int64_t* __restrict__ chunks, const int* __restrict__ seg_group, int nseg,
                                                           float2* __restrict__ partial, const AdamGroup* __restrict__ groups,
                                                           AdamGroupArgs garg, const float* __restrict__ clip, int skip_nonfinite) {
  const float gscale = clip ? clip[1] : 1.f;
  if (clip && skip_nonfinite && clip[2] != 0.f) return;
  __shared__ float2 red[4];
  const int64_t start = chunks[blockIdx.x * 3ll + 0], elems = chunks[blockIdx.x * 3ll + 1], seg = chunks[blockIdx.x * 3ll + 2];
  // a row that does not describe a chunk inside the buffers is not followed (uniform)
  if (start < 0 || elems < 0 || elems > LAMB_CHUNK || start + elems > n || seg < 0 || seg >= nseg) return;
  const int gi = seg_group[seg];
  if (gi < 0) return;
  const AdamGroup G = groups ? groups[gi] : garg.g[gi];
  const int e4 = (int)(elems / 4);
  float sp = 0.f, su = 0.f;
#pragma unroll
  for (int it = 0; it < LAMB_CHUNK / 1024; ++it) {
    const int i = threadIdx.x + 256 * it;
    if (i < e4) {
      const int64_t e = start + 4ll * i;
      const float4 pp = *(const float4*)(p + e);
      const float4 gg4 = *(const float4*)(g + e);
      float4 mm = *(float4*)(m + e);
      float4 vv = *(float4*)(v + e);
      const float* pa = &pp.x; const float* ga = &gg4.x; float* ma = &mm.x; float* va = &vv.x;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float gr = ga[j] * gscale;
        ma[j] = G.beta1 * ma[j] + G.one_minus_beta1 * gr;
        va[j] = G.beta2 * va[j] + G.one_minus_beta2 * gr * gr;
        const float u = lamb_u(pa[j], ma[j], va[j], G);
        sp += pa[j] * pa[j];
        su += u * u;
      }
      *(float4*)(m + e) = mm;
      *(float4*)(v + e) = vv;
    }
  }
  sp = wave_sum(sp);
  su = wave_sum(su);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float2(sp, su);
  __syncthreads();
  if (threadIdx.x == 0)
    partial[blockIdx.x] = make_float2((red[0].x + red[1].x) + (red[2].x + red[3].x), (red[0].y + red[1].y) + (red[2].y + red[3].y));
}

// One workgroup per segment: the chunk sums in double, thread t taking chunks t, t + 256, ... in order
// (norm_finalize_kernel's arrangement).
__global__ void __launch_bounds__(256) lamb_ratio_kernel(const float2* __restrict__ partial, int nchunks,
                                                         const int64_t* __restrict__ seg_chunks, const int* __restrict__ seg_group,
                                                         float* __restrict__ trust, const AdamGroup* __restrict__ groups,
                                                         AdamGroupArgs garg, const float* __restrict__ clip, int skip_nonfinite) {
  if (clip && skip_nonfinite && clip[2] != 0.f) return;
  __shared__ double red[4][2];
  const int seg = blockIdx.x;
  const int gi = seg_group[seg];
  if (gi < 0) return;  // frozen: the row stays
  const int64_t first = seg_chunks[seg * 2ll + 0], cnt = seg_chunks[seg * 2ll + 1];
  if (first < 0 || cnt < 0 || first + cnt > nchunks) return;
  double sp = 0.0, su = 0.0;
  for (int64_t i = threadIdx.x; i < cnt; i += 256) {
    const float2 c = partial[first + i];
    sp += (double)c.x;
    su += (double)c.y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sp += __shfl_xor(sp, o, 64);
    su += __shfl_xor(su, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = sp;
    red[threadIdx.x >> 6][1] = su;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const AdamGroup G = groups ? groups[gi] : garg.g[gi];
    const double wn = sqrt((red[0][0] + red[1][0]) + (red[2][0] + red[3][0]));
    const double un = sqrt((red[0][1] + red[1][1]) + (red[2][1] + red[3][1]));
    float r = 1.f;
    if (lamb_adapts(G) && wn > 0.0 && un > 0.0) r = (float)(wn / un);
    trust[seg * 3ll + 0] = (float)wn;
    trust[seg * 3ll + 1] = (float)un;
    trust[seg * 3ll + 2] = r;
  }
}

__device__ __forceinline__ void lamb4(float4& pp, const float4& mm, const float4& vv, const AdamGroup& G, float lr_r) {
  float* pa = &pp.x; const float* ma = &mm.x; const float* va = &vv.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) pa[j] -= lr_r * lamb_u(pa[j], ma[j], va[j], G);
}

// The structure of adam_t_kernel and adam_kernel (optim.hip) in one launch form.
// ntiles > 0: blocks [0, ntiles) take one 64x64 tile of a registered 2-D weight (tmeta row {flat offset,
//   W^T offset in shadow_t, R, C, first tile, param group, segment}); the others stride over the rest
//   (fmeta row {flat start, elements, param group, first float4, segment}).
// ntiles == 0: every block strides over the n elements and finds its segment in seg_start.
template <bool EMA>
__global__ void __launch_bounds__(256) lamb_update_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                          uint16_t* __restrict__ shadow, uint16_t* __restrict__ shadow_t, int64_t n,
                                                          const int64_t* __restrict__ seg_start, const int* __restrict__ seg_group, int nseg,
                                                          const int64_t* __restrict__ tmeta, int nmat, int ntiles,
                                                          const int64_t* __restrict__ fmeta, int nflat, int64_t flat4,
                                                          const float* __restrict__ trust, const AdamGroup* __restrict__ groups,
                                                          AdamGroupArgs garg, const float* __restrict__ clip, int skip_nonfinite,
                                                          EmaArg<EMA> ea) {
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
      if (tmeta[mid * 7 + 4] <= blk) lo = mid; else hi = mid - 1;
    }
    const int64_t soff = tmeta[lo * 7 + 0], doff = tmeta[lo * 7 + 1];
    const int R = (int)tmeta[lo * 7 + 2], C = (int)tmeta[lo * 7 + 3];
    const int gi = (int)tmeta[lo * 7 + 5];
    const int local = blk - (int)tmeta[lo * 7 + 4];
    const int tc = C / 64;
    const int r0 = (local / tc) * 64, c0 = (local % tc) * 64;
    if (gi < 0) return;  // frozen: master, shadow and W^T unchanged
    const AdamGroup G = groups ? groups[gi] : garg.g[gi];
    const float lr_r = G.lr * trust[tmeta[lo * 7 + 6] * 3 + 2];
    const int cq = (tid & 15) * 4;
    float4 pn[EMA ? 4 : 1];  // EMA: the four new values, averaged after the unrolled updates
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = (tid >> 4) + 16 * it;
      const int64_t e = soff + (int64_t)(r0 + row) * C + c0 + cq;
      float4 pp = *(float4*)(p + e);
      const float4 mm = *(const float4*)(m + e);
      const float4 vv = *(const float4*)(v + e);
      lamb4(pp, mm, vv, G, lr_r);
      *(float4*)(p + e) = pp;
      if constexpr (EMA) pn[it] = pp;
      const uint32_t lo2 = pack2bf(pp.x, pp.y), hi2 = pack2bf(pp.z, pp.w);
      *(uint2*)(shadow + e) = make_uint2(lo2, hi2);
      tile[row][cq >> 1] = lo2;
      tile[row][(cq >> 1) + 1] = hi2;
    }
    if constexpr (EMA) {
      if (ea.a.buf != nullptr) {
#pragma unroll
        for (int it = 0; it < 4; ++it)
          ema4(ea.a.buf, soff + (int64_t)(r0 + (tid >> 4) + 16 * it) * C + c0 + cq, pn[it], dw);
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
  const int64_t total4 = ntiles > 0 ? flat4 : n / 4;
  for (int64_t i = ((int64_t)blockIdx.x - ntiles) * 256 + tid; i < total4; i += nblk * 256) {
    int64_t e;
    int gi, seg;
    if (ntiles > 0) {
      int lo = 0, hi = nflat - 1;  // range holding float4 i
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (fmeta[mid * 5 + 3] <= i) lo = mid; else hi = mid - 1;
      }
      gi = (int)fmeta[lo * 5 + 2];
      seg = (int)fmeta[lo * 5 + 4];
      e = fmeta[lo * 5 + 0] + (i - fmeta[lo * 5 + 3]) * 4;
    } else {
      e = i * 4;
      int lo = 0, hi = nseg - 1;  // the segment containing e (segments are 4-element aligned by construction)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_start[mid] <= e) lo = mid; else hi = mid - 1;
      }
      gi = seg_group[lo];
      seg = lo;
    }
    if (gi < 0) continue;  // frozen / padding
    const AdamGroup G = groups ? groups[gi] : garg.g[gi];
    const float lr_r = G.lr * trust[seg * 3ll + 2];
    float4 pp = *(float4*)(p + e);
    const float4 mm = *(const float4*)(m + e);
    const float4 vv = *(const float4*)(v + e);
    lamb4(pp, mm, vv, G, lr_r);
    *(float4*)(p + e) = pp;
    if (shadow) *(uint2*)(shadow + e) = make_uint2(pack2bf(pp.x, pp.y), pack2bf(pp.z, pp.w));
    if constexpr (EMA) {
      if (ea.a.buf != nullptr) ema4(ea.a.buf, e, pp, dw);
    }
  }
}

}  // namespace
}  // namespace pvr

extern "C" hipError_t pvr_lamb_moments(const float* p, const float* g, float* m, float* v, int64_t n, const int64_t* chunks,
                                       int nchunks, const int* seg_group, int nseg, float* partial, const pvr::AdamGroup* groups,
                                       const pvr::AdamGroup* host_groups, int ngroups, const float* clip, int skip_nonfinite,
                                       hipStream_t s) {
  using namespace pvr;
  if (nchunks <= 0) return hipSuccess;
  if (n <= 0 || n % 4 != 0 || nseg <= 0) return hipErrorInvalidValue;
  AdamGroupArgs ga{};
  if (!groups && !adam_group_args(host_groups, ngroups, ga)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)nchunks), dim3(256), 0, s, p, g, m, v, n, chunks, seg_group, nseg,
                     (float2*)partial, groups, ga, clip, skip_nonfinite);
  return hipGetLastError();
}

extern "C" hipError_t pvr_lamb_ratio(const float* partial, int nchunks, const int64_t* seg_chunks, const int* seg_group, int nseg,
                                     float* trust, const pvr::AdamGroup* groups, const pvr::AdamGroup* host_groups, int ngroups,
                                     const float* clip, int skip_nonfinite, hipStream_t s) {
  using namespace pvr;
  if (nseg <= 0 || nchunks < 0) return hipErrorInvalidValue;
  AdamGroupArgs ga{};
  if (!groups && !adam_group_args(host_groups, ngroups, ga)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lamb_ratio_kernel, dim3((unsigned)nseg), dim3(256), 0, s, (const float2*)partial, nchunks, seg_chunks, seg_group,
                     trust, groups, ga, clip, skip_nonfinite);
  return hipGetLastError();
}

extern "C" hipError_t pvr_lamb_update(float* p, const float* m, const float* v, uint16_t* shadow, uint16_t* shadow_t, int64_t n,
                                      const int64_t* seg_start, const int* seg_group, int nseg, const int64_t* tmeta, int nmat,
                                      int ntiles, const int64_t* fmeta, int nflat, int64_t flat4, const float* trust,
                                      const pvr::AdamGroup* groups, const pvr::AdamGroup* host_groups, int ngroups, const float* clip,
                                      int skip_nonfinite, pvr::AdamEma ema, hipStream_t s) {
  using namespace pvr;
  int64_t fb;
  if (ntiles > 0) {
    if (nmat <= 0 || nflat <= 0 || !tmeta || !fmeta || !shadow || !shadow_t) return hipErrorInvalidValue;
    fb = (flat4 + 255) / 256;
    if (fb > 1024) fb = 1024;
  } else {
    if (ntiles < 0 || nseg <= 0 || !seg_start || !seg_group) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    if (n % 4 != 0) return hipErrorInvalidValue;
    fb = (n / 4 + 255) / 256;
    if (fb > 8192) fb = 8192;
  }
  if (fb < 1) fb = 1;
  AdamGroupArgs ga{};
  if (!groups && !adam_group_args(host_groups, ngroups, ga)) return hipErrorInvalidValue;
  if (ema.buf) {
    hipLaunchKernelGGL(lamb_update_kernel<true>, dim3((unsigned)(ntiles + fb)), dim3(256), 0, s, p, m, v, shadow, shadow_t, n,
                       seg_start, seg_group, nseg, tmeta, nmat, ntiles, fmeta, nflat, flat4, trust, groups, ga, clip, skip_nonfinite,
                       EmaArg<true>{ema});
  } else {
    hipLaunchKernelGGL(lamb_update_kernel<false>, dim3((unsigned)(ntiles + fb)), dim3(256), 0, s, p, m, v, shadow, shadow_t, n,
                       seg_start, seg_group, nseg, tmeta, nmat, ntiles, fmeta, nflat, flat4, trust, groups, ga, clip, skip_nonfinite,
                       EmaArg<false>{});
  }
  return hipGetLastError();
}
