// Fused binary cross-entropy with logits against mixed / smoothed label rows (DeiT-III, timm's
// BinaryCrossEntropy): the sigmoid-loss counterpart of xent.hip's xent_soft_kernel. One pass over a
// logit row produces the row loss, d(loss)/d(logits) and the argmax == label flag; unlike softmax the
// gradient of a class depends on its own logit only, so nothing is reduced before it is written.
#include "common.h"
#include "kernels.h"

namespace pvr {
namespace {

// Target of class c: q = (1 - eps) * ((c == ya) * lam + (c == yb) * (1 - lam)) + eps / C, xent_soft_kernel's
// expression; thr >= 0 binarises it (t = q > thr, timm's target_threshold). Per element, in fp32:
//   l = max(x, 0) - x t + log1p(exp(-|x|))    (= log(1 + exp(x)) - x t without overflow)
//   d = sigmoid(x) - t, sigmoid from the same exp(-|x|): 1 / (1 + e) for x >= 0, e / (1 + e) below
// expf / log1pf, not the fast intrinsics: past |x| ~ 17 log(1 + e) is 0 in fp32 while log1p(e) = e is the
// whole loss of a confidently right class. The row sum has a fixed order: a strided partial per thread,
// the wave butterfly, then the four waves in order through LDS.
__global__ void __launch_bounds__(256) bce_kernel(const float* __restrict__ logits, int64_t ld, const int64_t* __restrict__ ya_,
                                                   const int64_t* __restrict__ yb_, const float* __restrict__ lam_, float eps, float thr,
                                                   int B, int C, float row_scale, float* __restrict__ loss_rows,
                                                   float* __restrict__ dlogits, int* __restrict__ correct, float grad_scale) {
  __shared__ float smax[4], ssum[4];
  __shared__ int sidx[4];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = logits + (int64_t)b * ld;
  const int64_t ya = ya_[b], yb = yb_[b];
  const bool valid = ya >= 0 && ya < C && yb >= 0 && yb < C;  // as xent_soft_kernel: such rows contribute nothing
  const float lam = lam_[b], oml = 1.0f - lam, ome = 1.0f - eps, eoc = eps / (float)C;
  float* dl = dlogits ? dlogits + (int64_t)b * C : nullptr;
  float m = -INFINITY, s = 0.f;
  int mi = 0x7FFFFFFF;
  // Four strided trips at a time, their loads issued together: a trip is one load and then a long dependent
  // chain (exp, log1p, a division), and one trip after the other pays the memory latency once per trip.
  // Each thread still visits its columns in rising order, so the order of its partial sum is that of a plain loop.
  for (int c0 = tid; c0 < C; c0 += 4 * 256) {
    float xv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) xv[k] = c0 + k * 256 < C ? x[c0 + k * 256] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = c0 + k * 256;
      if (c >= C) break;
      const float v = xv[k];
      if (v > m || (v == m && c < mi)) { m = v; mi = c; }  // first argmax, xent_kernel's tie rule
      const float w = (c == ya ? lam : 0.f) + (c == yb ? oml : 0.f);
      const float q = __fadd_rn(__fmul_rn(ome, w), eoc);  // two roundings whatever -ffp-contract says: q > thr is the same on every build
      const float t = thr >= 0.f ? (q > thr ? 1.f : 0.f) : q;
      const float e = expf(-fabsf(v));
      s += fmaxf(v, 0.f) - v * t + log1pf(e);
      if (dl) {
        const float sig = v >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        dl[c] = valid ? (sig - t) * grad_scale : 0.f;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oi = __shfl_xor(mi, o, 64);
    if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
  }
  s = wave_sum(s);
  if (lane == 0) { smax[wave] = m; sidx[wave] = mi; ssum[wave] = s; }
  __syncthreads();
  if (tid == 0) {
    m = smax[0]; mi = sidx[0];
    for (int w = 1; w < 4; ++w)
      if (smax[w] > m || (smax[w] == m && sidx[w] < mi)) { m = smax[w]; mi = sidx[w]; }
    s = ssum[0] + ssum[1] + ssum[2] + ssum[3];
    loss_rows[b] = valid ? row_scale * s : 0.f;
    if (correct) correct[b] = mi == (int)ya ? 1 : 0;  // the sample's own label
  }
}

}  // namespace
}  // namespace pvr

extern "C" hipError_t pvr_bce(const float* logits, int64_t ld, const int64_t* ya, const int64_t* yb, const float* lam, float eps,
                              float thr, int B, int C, float row_scale, float* loss_rows, float* dlogits, int* correct,
                              float grad_scale, hipStream_t s) {
  using namespace pvr;
  if (B <= 0) return hipSuccess;
  if (C <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bce_kernel, dim3(B), dim3(256), 0, s, logits, ld, ya, yb, lam, eps, thr, B, C, row_scale, loss_rows, dlogits,
                     correct, grad_scale);
  return hipGetLastError();
}
