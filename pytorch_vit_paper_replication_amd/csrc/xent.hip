// Fused softmax cross-entropy for the classifier logits (reference GM/engine.py:53, :73-74;
// SURVEY.md K13 + K16): one pass produces the per-row loss, d(loss)/d(logits) for the mean
// reduction, and the argmax==label flag per row for the accuracy metric, so the engine does not
// need a separate softmax/argmax/eq/sum chain or a host sync per batch.
#include "common.h"
#include "kernels.h"

namespace pvr {
namespace {

__global__ void __launch_bounds__(256) xent_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                    int B, int C, float* __restrict__ loss_rows, float* __restrict__ dlogits,
                                                    int* __restrict__ correct, float grad_scale) {
  __shared__ float smax[4], ssum[4];
  __shared__ int sidx[4];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (int64_t)b * ld;
  // max and first argmax
  float m = -INFINITY;
  int mi = 0x7FFFFFFF;
  for (int c = tid; c < C; c += 256) {
    const float v = x[c];
    if (v > m || (v == m && c < mi)) { m = v; mi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  if (lane == 0) { smax[wave] = m; sidx[wave] = mi; }
  __syncthreads();
  m = smax[0]; mi = sidx[0];
  for (int w = 1; w < 4; ++w)
    if (smax[w] > m || (smax[w] == m && sidx[w] < mi)) { m = smax[w]; mi = sidx[w]; }
  float s = 0.f;
  for (int c = tid; c < C; c += 256) s += __expf(x[c] - m);
  s = wave_sum(s);
  if (lane == 0) ssum[wave] = s;
  __syncthreads();
  s = ssum[0] + ssum[1] + ssum[2] + ssum[3];
  const float lse = m + __logf(s);
  const int64_t y = labels[b];
  const bool valid = y >= 0 && y < C;  // out-of-range labels (e.g. ignore_index) contribute nothing
  if (tid == 0) {
    loss_rows[b] = valid ? lse - x[y] : 0.f;
    if (correct) correct[b] = mi == (int)y ? 1 : 0;  // per-row flag: no zeroed counter needed
  }
  if (dlogits) {
    const float inv = 1.f / s;
    for (int c = tid; c < C; c += 256) {
      float p = __expf(x[c] - m) * inv;
      if (c == y) p -= 1.f;
      dlogits[(int64_t)b * C + c] = valid ? p * grad_scale : 0.f;
    }
  }
}

// xent_kernel for soft target rows q = (1 - eps) * (lam * onehot(ya) + (1 - lam) * onehot(yb)) + eps / C
// (mixup / CutMix label pairs, label smoothing). Max, exp sum, lse and p are xent_kernel's operations
// in its order; the loop that sums the exponentials also sums the logits:
//   loss = -sum_c q_c (x_c - lse) = lse - (1 - eps) * (lam * x[ya] + (1 - lam) * x[yb]) - (eps / C) * sum_c x_c
// With lam = 1, eps = 0, yb = ya every extra term is an exact 0 and p - q is the fma xent_kernel's
// label column compiles to, so loss rows and dlogits carry its bits.
__global__ void __launch_bounds__(256) xent_soft_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ ya_,
                                                         const int64_t* __restrict__ yb_, const float* __restrict__ lam_, float eps,
                                                         int B, int C, float* __restrict__ loss_rows, float* __restrict__ dlogits,
                                                         int* __restrict__ correct, float grad_scale) {
  __shared__ float smax[4], ssum[4], sx[4];
  __shared__ int sidx[4];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (int64_t)b * ld;
  // max and first argmax
  float m = -INFINITY;
  int mi = 0x7FFFFFFF;
  for (int c = tid; c < C; c += 256) {
    const float v = x[c];
    if (v > m || (v == m && c < mi)) { m = v; mi = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  if (lane == 0) { smax[wave] = m; sidx[wave] = mi; }
  __syncthreads();
  m = smax[0]; mi = sidx[0];
  for (int w = 1; w < 4; ++w)
    if (smax[w] > m || (smax[w] == m && sidx[w] < mi)) { m = smax[w]; mi = sidx[w]; }
  float s = 0.f, t = 0.f;
  for (int c = tid; c < C; c += 256) {
    s += __expf(x[c] - m);
    t += x[c];
  }
  s = wave_sum(s);
  t = wave_sum(t);
  if (lane == 0) { ssum[wave] = s; sx[wave] = t; }
  __syncthreads();
  s = ssum[0] + ssum[1] + ssum[2] + ssum[3];
  t = sx[0] + sx[1] + sx[2] + sx[3];
  const float lse = m + __logf(s);
  const int64_t ya = ya_[b], yb = yb_[b];
  const bool valid = ya >= 0 && ya < C && yb >= 0 && yb < C;  // as xent_kernel: such rows contribute nothing
  const float lam = lam_[b], oml = 1.0f - lam, ome = 1.0f - eps, eoc = eps / (float)C;
  if (tid == 0) {
    // without smoothing the logit sum carries no weight: not 0 * t, which is NaN on a row with a
    // masked (-inf) class, where t = -inf
    const float smooth = eoc != 0.f ? eoc * t : 0.f;
    loss_rows[b] = valid ? lse - ome * (lam * x[ya] + oml * x[yb]) - smooth : 0.f;
    if (correct) correct[b] = mi == (int)ya ? 1 : 0;  // the sample's own label
  }
  if (dlogits) {
    const float inv = 1.f / s;
    for (int c = tid; c < C; c += 256) {
      const float w = (c == ya ? lam : 0.f) + (c == yb ? oml : 0.f);
      const float q = ome * w + eoc;
      const float p = __fmaf_rn(__expf(x[c] - m), inv, -q);  // softmax - q, one rounding
      dlogits[(int64_t)b * C + c] = valid ? p * grad_scale : 0.f;
    }
  }
}

}  // namespace
}  // namespace pvr

extern "C" hipError_t pvr_xent_soft(const float* logits, int64_t ld, const int64_t* ya, const int64_t* yb, const float* lam, float eps,
                                    int B, int C, float* loss_rows, float* dlogits, int* correct, float grad_scale, hipStream_t s) {
  using namespace pvr;
  if (B <= 0) return hipSuccess;
  if (C <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(xent_soft_kernel, dim3(B), dim3(256), 0, s, logits, ld, ya, yb, lam, eps, B, C, loss_rows, dlogits, correct,
                     grad_scale);
  return hipGetLastError();
}

extern "C" hipError_t pvr_xent(const float* logits, int64_t ld, const int64_t* labels, int B, int C, float* loss_rows,
                               float* dlogits, int* correct, float grad_scale, hipStream_t s) {
  using namespace pvr;
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(xent_kernel, dim3(B), dim3(256), 0, s, logits, ld, labels, B, C, loss_rows, dlogits, correct, grad_scale);
  return hipGetLastError();
}
