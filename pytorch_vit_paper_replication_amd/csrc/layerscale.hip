// LayerScale (Touvron et al., "Going deeper with Image Transformers") as a reparameterisation of the
// last Linear of each residual branch: g * (a W^T + b) = a (diag(g) W)^T + g * b. The fold writes the
// bf16 copies of diag(g) W that the GEMMs read in place of W's shadows; the unfold turns the gradients
// the unchanged kernels deliver for the folded pair into those of W, b and g. Both are memory-bound
// passes; no GEMM, LayerNorm or attention kernel knows about the scale.
#include "common.h"
#include "kernels.h"

namespace pvr {
namespace {

// One launch over every scaled weight. meta int64 [nmat][8] = {W offset, g offset, b offset (all in
// `master`), R, C, offset in w16 / wt16, offset in bhat, tile prefix}; R, C and the offsets are
// multiples of 8 (host-checked), so every 8-element group is whole: inside the matrix or outside it.
//   w16[i][j] = bf16_rne(fl32(g[i] * W[i][j])), wt16[j][i] the same values, bhat[i] = fl32(g[i] * b[i]).
// 64x64 tiles through LDS held as bf16 pairs (33-word rows), as transpose_batched_kernel.
__global__ void __launch_bounds__(256) layerscale_fold_kernel(const float* __restrict__ master, uint16_t* __restrict__ w16,
                                                               uint16_t* __restrict__ wt16, float* __restrict__ bhat,
                                                               const int64_t* __restrict__ meta, int nmat) {
  __shared__ uint32_t tile[64][33];
  const int blk = blockIdx.x;
  int lo = 0, hi = nmat - 1;  // last t with tile prefix <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (meta[mid * 8 + 7] <= blk) lo = mid; else hi = mid - 1;
  }
  const int64_t* row_meta = meta + lo * 8;
  const float* W = master + row_meta[0];
  const float* g = master + row_meta[1];
  const float* b = master + row_meta[2];
  const int R = (int)row_meta[3], C = (int)row_meta[4];
  uint16_t* out = w16 + row_meta[5];
  uint16_t* out_t = wt16 + row_meta[5];
  const int local = blk - (int)row_meta[7];
  const int tc = (C + 63) / 64;
  const int r0 = (local / tc) * 64, c0 = (local % tc) * 64;
  const int tid = threadIdx.x;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int row = tid / 8 + 32 * it, ch = tid % 8;
    const int r = r0 + row, c = c0 + ch * 8;
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (r < R && c < C) {
      const float gi = g[r];
      const float4 x = *(const float4*)(W + (int64_t)r * C + c);
      const float4 y = *(const float4*)(W + (int64_t)r * C + c + 4);
      q.x = pack2bf(gi * x.x, gi * x.y); q.y = pack2bf(gi * x.z, gi * x.w);
      q.z = pack2bf(gi * y.x, gi * y.y); q.w = pack2bf(gi * y.z, gi * y.w);
      *(uint4*)(out + (int64_t)r * C + c) = q;
    }
    tile[row][ch * 4 + 0] = q.x; tile[row][ch * 4 + 1] = q.y;
    tile[row][ch * 4 + 2] = q.z; tile[row][ch * 4 + 3] = q.w;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int idx = tid + 256 * it;
    const int cc = idx / 8, rch = idx % 8;  // output row (input column) cc, input rows rch*8 .. +7
    if (c0 + cc < C && r0 + rch * 8 < R) {
      uint32_t h[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = (tile[rch * 8 + j][cc >> 1] >> ((cc & 1) * 16)) & 0xFFFFu;
      uint4 o;
      o.x = h[0] | (h[1] << 16); o.y = h[2] | (h[3] << 16); o.z = h[4] | (h[5] << 16); o.w = h[6] | (h[7] << 16);
      *(uint4*)(out_t + (int64_t)(c0 + cc) * R + r0 + rch * 8) = o;
    }
  }
  if (c0 == 0 && tid < 64 && r0 + tid < R) bhat[row_meta[6] + r0 + tid] = g[r0 + tid] * b[r0 + tid];
}

// acc + fl32(g * d): the product rounded on its own, so a gradient unfolded into a zeroed buffer is the fp32
// product bit for bit and one added to a gradient that is already there is torch's two operations. The build's
// -ffp-contract=fast lets the backend fuse a multiply into an add whatever a pragma says; the empty asm makes
// the product opaque to it (it emits nothing).
PVR_DEV float scaled_add(float acc, float g, float d) {
  float p = g * d;
  asm volatile("" : "+v"(p));
  return acc + p;
}

// One workgroup per row i of a scaled Linear (W [R][C], b [R], scale g [R]); dWh [R][C] and dbh [R] are the
// gradients the GEMM / column-sum kernels delivered for the folded pair. Any destination may be null:
//   gW[i][j] += fl32(g[i] * dWh[i][j]),  gb[i] += fl32(g[i] * dbh[i]),
//   gg[i]    += fl32(sum_j dWh[i][j] * W[i][j] + dbh[i] * b[i])
// The dot product runs in double: a strided partial per thread, a wave butterfly, then the four waves
// through LDS in wave order. No atomics: the same bits on every run. VEC: every row is 16-byte aligned.
template <bool VEC>
__global__ void __launch_bounds__(256) layerscale_unfold_kernel(const float* __restrict__ dWh, const float* __restrict__ dbh,
                                                                 const float* __restrict__ W, const float* __restrict__ b,
                                                                 const float* __restrict__ g, float* __restrict__ gW,
                                                                 float* __restrict__ gb, float* __restrict__ gg, int C) {
  __shared__ double red[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float gi = g[i];
  const float* drow = dWh + (int64_t)i * C;
  const float* wrow = W + (int64_t)i * C;
  float* grow = gW ? gW + (int64_t)i * C : nullptr;
  double acc = 0.0;
  if (gW || gg) {
    if (VEC) {
      for (int c4 = tid; c4 < C / 4; c4 += 256) {
        const float4 d = ((const float4*)drow)[c4];
        if (gg) {
          const float4 w = ((const float4*)wrow)[c4];
          acc += (double)d.x * (double)w.x; acc += (double)d.y * (double)w.y;
          acc += (double)d.z * (double)w.z; acc += (double)d.w * (double)w.w;
        }
        if (grow) {
          float4 o = ((float4*)grow)[c4];
          o.x = scaled_add(o.x, gi, d.x); o.y = scaled_add(o.y, gi, d.y);
          o.z = scaled_add(o.z, gi, d.z); o.w = scaled_add(o.w, gi, d.w);
          ((float4*)grow)[c4] = o;
        }
      }
    } else {
      for (int c = tid; c < C; c += 256) {
        const float d = drow[c];
        if (gg) acc += (double)d * (double)wrow[c];
        if (grow) grow[c] = scaled_add(grow[c], gi, d);
      }
    }
  }
  if (gg) {  // (uniform over the grid: every thread reaches the barrier)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      const double t = ((red[0] + red[1]) + red[2]) + red[3] + (double)dbh[i] * (double)b[i];
      gg[i] += (float)t;
    }
  }
  if (gb && tid == 0) gb[i] = scaled_add(gb[i], gi, dbh[i]);
}

}  // namespace
}  // namespace pvr

extern "C" hipError_t pvr_layerscale_fold(const float* master, uint16_t* w16, uint16_t* wt16, float* bhat, const int64_t* meta,
                                          int nmat, int total_tiles, hipStream_t s) {
  using namespace pvr;
  if (nmat <= 0 || total_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(layerscale_fold_kernel, dim3(total_tiles), dim3(256), 0, s, master, w16, wt16, bhat, meta, nmat);
  return hipGetLastError();
}

extern "C" hipError_t pvr_layerscale_unfold(const float* dWh, const float* dbh, const float* W, const float* b, const float* g,
                                            float* gW, float* gb, float* gg, int R, int C, int vec, hipStream_t s) {
  using namespace pvr;
  if (R <= 0 || (!gW && !gb && !gg)) return hipSuccess;
  if (C <= 0 || (vec && C % 4)) return hipErrorInvalidValue;
  if (vec)
    hipLaunchKernelGGL(layerscale_unfold_kernel<true>, dim3(R), dim3(256), 0, s, dWh, dbh, W, b, g, gW, gb, gg, C);
  else
    hipLaunchKernelGGL(layerscale_unfold_kernel<false>, dim3(R), dim3(256), 0, s, dWh, dbh, W, b, g, gW, gb, gg, C);
  return hipGetLastError();
}
