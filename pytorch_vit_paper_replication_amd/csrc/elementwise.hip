// Memory-bound helper kernels (16-B vector accesses throughout, SURVEY.md K1-K4, K11 bias-grad):
//   * flat fp32 -> bf16 shadow cast of the parameter store
//   * bias-gradient column sums, optionally fused with the dropout-mask backward
//   * patch embedding: im2col gather (fp32 image -> bf16 patch rows), CLS rows, and the backward
//     reduction of the embedding-dropout / position-embedding / CLS gradients;
//   * patch dropout: the per-sample keep table (ranks of counter-hash keys), the gathered position
//     addend, and the KEEP instantiations of the patchify kernels and of the backward's first pass;
//   * random erasing: the ERASE instantiations of the patchify kernels and the fill's noise as a kernel.
#include "common.h"
#include "kernels.h"

namespace pvr {
namespace {

__global__ void __launch_bounds__(256) cast_f32_bf16_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, int64_t n) {
  const int64_t n4 = n / 4;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 v = ((const float4*)in)[i];
    uint2 o;
    o.x = pack2bf(v.x, v.y);
    o.y = pack2bf(v.z, v.w);
    ((uint2*)out)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t i = n4 * 4 + threadIdx.x;
    out[i] = f2bf(in[i]);
  }
}

// dY [rows][N] (row stride ld) -> db[N] += column sums of (mask * dY); if dz != null also writes
// the masked gradient dz (= dropout backward) with row stride ld_dz. row_mul: the mask of row r is that of row
// r * row_mul of a larger [rows * row_mul][N] tensor (1: this one; > 1: its class-token rows, compact).
// Q8: also the fp8 copy (qfmt 1 e5m2, 0 e4m3) of the (masked) gradient, q[r][n] = fp8(v * *qscale), and its amax record
// (the fp8 dgrad operand of the same tensor whose column sums are the bias gradient: one read, two uses)
// DP: the branch's drop-path row scale too, v = s[r / dp_rows] * mask * scale * dy (s = 0 or dp_scale per
// sample; independent of row_mul); the element and row scales fold into one fp32 factor per row.
template <bool Q8, bool DP = false>
__global__ void __launch_bounds__(256) colsum_kernel(const uint16_t* __restrict__ dy, int64_t ld, int rows, int N,
                                                      float* __restrict__ db, uint16_t* __restrict__ dz, int64_t ld_dz,
                                                      const uint64_t* seed_ptr, uint64_t seed_off, uint32_t thr, float scale,
                                                      uint8_t* __restrict__ qout, int64_t ld_q, const float* __restrict__ qscale,
                                                      unsigned* __restrict__ amax, int qfmt, float* __restrict__ part, int row_mul,
                                                      const uint64_t* dp_seed_ptr, uint64_t dp_off, uint32_t dp_thr, float dp_scale,
                                                      int dp_rows) {
  __shared__ float red[4][64 * 8];
  const float qs = Q8 ? *qscale : 1.f;
  float qam = 0.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + lane;  // 8-column chunk
  const bool act = c * 8 < N;
  const uint64_t seed = thr ? (*seed_ptr + seed_off) : 0ull;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t dkey = 0u;
  float dfk = 0.f;
  if constexpr (DP) {
    dkey = rng_key(*dp_seed_ptr + dp_off);
    dfk = (thr ? scale : 1.f) * dp_scale;
  }
  if (act) {
    // 4 rows per trip with their loads issued together (clamped rows, so the loads are
    // unconditional and the compiler counts them instead of draining vmcnt per row)
    constexpr int U = 4;
    const int stride = gridDim.y * 4;
    for (int r0 = blockIdx.y * 4 + wave; r0 < rows; r0 += U * stride) {
      uint4 q[U];
#pragma unroll
      for (int u = 0; u < U; ++u) q[u] = *(const uint4*)(dy + (int64_t)min(r0 + u * stride, rows - 1) * ld + c * 8);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int r = r0 + u * stride;
        if (r >= rows) break;
        const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
        float v[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[2 * j] = bf2f(w[j] & 0xFFFF);
          v[2 * j + 1] = bf2f(w[j] >> 16);
        }
        if constexpr (DP) {
          const float rf = rng_keep_32(dkey, (uint32_t)r / (uint32_t)dp_rows, dp_thr) ? dfk : 0.f;  // wave-uniform
#pragma unroll
          for (int j = 0; j < 8; j += 2) {
            bool k0 = true, k1 = true;
            if (thr) rng_keep2(seed, (uint64_t)r * row_mul * N + c * 8 + j, thr, k0, k1);
            v[j] = k0 ? v[j] * rf : 0.f;
            v[j + 1] = k1 ? v[j + 1] * rf : 0.f;
          }
        } else if (thr) {
#pragma unroll
          for (int j = 0; j < 8; j += 2) {
            bool k0, k1;
            rng_keep2(seed, (uint64_t)r * row_mul * N + c * 8 + j, thr, k0, k1);
            v[j] = k0 ? v[j] * scale : 0.f;
            v[j + 1] = k1 ? v[j + 1] * scale : 0.f;
          }
        }
        if (dz) {
          uint4 o;
          o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]);
          o.z = pack2bf(v[4], v[5]); o.w = pack2bf(v[6], v[7]);
          *(uint4*)(dz + (int64_t)r * ld_dz + c * 8) = o;
          if constexpr (DP) {
            // as in ln_bwd_kernel's drop-path instantiations (layernorm.hip): the bias gradient of a
            // drop-path branch sums the bf16 dz values that its weight-gradient GEMM reads
            const uint32_t ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              v[2 * j] = bf2f(ow[j] & 0xFFFF);
              v[2 * j + 1] = bf2f(ow[j] >> 16);
            }
          }
        }
        if constexpr (Q8) {
          float vm = 0.f;
#pragma unroll
          for (int j = 0; j < 8; ++j) vm = nan_max(vm, fabsf(v[j]));
          qam = nan_max(qam, vm);
          *(uint2*)(qout + (int64_t)r * ld_q + c * 8) = pack8_fp8_fast_rt(qfmt, v, qs, vm);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += v[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[wave][lane * 8 + j] = acc[j];
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 8; i += 256) {
    const int col = blockIdx.x * 64 * 8 + i;
    if (col < N && part)  // deterministic mode: this row group's partial (rows_reduce sums them in order)
      part[(int64_t)blockIdx.y * N + col] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
    else if (col < N && db)
      atomicAdd(db + col, red[0][i] + red[1][i] + red[2][i] + red[3][i]);
  }
  if constexpr (Q8) {  // one amax atomic per workgroup
    qam = wave_max_nan(qam);
    __syncthreads();  // red[] reads above are done: reuse red[0][0..3]
    if (lane == 0) red[0][wave] = qam;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float m = nan_max(nan_max(red[0][0], red[0][1]), nan_max(red[0][2], red[0][3]));
      if (!(m <= 0.f)) atomicMax(amax, __float_as_uint(m));
    }
  }
}

// s[b] = drop-path scale of sample b at a site: 0 (dropped) or scale (see DropSite in kernels.h)
__global__ void __launch_bounds__(256) drop_path_scale_kernel(const uint64_t* seed_ptr, uint64_t off, uint32_t thr, float scale,
                                                               float* __restrict__ out, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B) out[b] = rng_keep(*seed_ptr + off, (uint64_t)b, thr) ? scale : 0.f;
}

// Patch dropout: which n_keep of a sample's np patches a training step keeps. The key of patch j of
// sample b is the full 32-bit rng_hash(*seed_ptr + off, b * np + j) (B * np < 2^32, host-checked: the
// index's high word is 0); the sample keeps the n_keep smallest (key, j) pairs, in ascending patch order:
//   keep[b][s] = index of the s-th kept patch (strictly ascending), inv[b][j] = slot s of patch j or -1.
// One workgroup per sample, keys in LDS (np <= PK_MAX). The rank of a patch is the number of smaller
// pairs (np reads per patch, np^2 / 256 per thread: microseconds at np = 196 or 576); the ranks are a
// permutation of 0 .. np - 1, so exactly n_keep patches have rank < n_keep. Their flags go to LDS as
// one ballot word pair per wave and trip, and the compact slot is the popcount of the flags below j.
constexpr int PK_MAX = 4096;
__global__ void __launch_bounds__(256) patch_keep_kernel(const uint64_t* seed_ptr, uint64_t off, int np, int n_keep,
                                                          int* __restrict__ keep, int* __restrict__ inv) {
  __shared__ uint32_t keys[PK_MAX];
  __shared__ uint32_t flags[PK_MAX / 32];
  const int b = blockIdx.x;
  const uint32_t key = rng_key(*seed_ptr + off);
  for (int j = threadIdx.x; j < np; j += 256) keys[j] = rng_mix32(((uint32_t)b * (uint32_t)np + (uint32_t)j) ^ key);
  __syncthreads();
  const int trips = (np + 255) / 256;  // uniform: every lane takes part in every ballot
  for (int t = 0; t < trips; ++t) {
    const int j = t * 256 + threadIdx.x;
    bool kept = false;
    if (j < np) {
      const uint32_t kj = keys[j];
      int rank = 0;
      for (int i = 0; i < np; ++i) {
        const uint32_t ki = keys[i];
        rank += (ki < kj || (ki == kj && i < j)) ? 1 : 0;
      }
      kept = rank < n_keep;
    }
    const uint64_t m = __builtin_amdgcn_ballot_w64(kept);
    if ((threadIdx.x & 63) == 0) {  // patches j .. j + 63 (flags past np are 0)
      flags[j >> 5] = (uint32_t)m;
      flags[(j >> 5) + 1] = (uint32_t)(m >> 32);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < np; j += 256) {
    const uint32_t fw = flags[j >> 5];
    int slot = __builtin_popcount(fw & ((1u << (j & 31)) - 1u));
    for (int w = 0; w < (j >> 5); ++w) slot += __builtin_popcount(flags[w]);
    const bool kept = (fw >> (j & 31)) & 1u;
    inv[(int64_t)b * np + j] = kept ? slot : -1;
    if (kept && slot < n_keep) keep[(int64_t)b * n_keep + slot] = j;
  }
}

// The embedding GEMM's position addend under patch dropout: out [B][n_keep + 1][D] fp32 with row
// 1 + s of sample b = pos[keep[b][s] + 1] (pos [np + 1][D]; row 0 = pos[0], which the GEMM does not read:
// cls_rows_kernel adds it). One thread per float4.
__global__ void __launch_bounds__(256) pos_gather_kernel(const float* __restrict__ pos, const int* __restrict__ keep,
                                                          float* __restrict__ out, int B, int np, int n_keep, int D) {
  const int d4 = D / 4;
  const int64_t total = (int64_t)B * (n_keep + 1) * d4;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % d4);
    const int64_t r = i / d4;
    const int n = (int)(r % (n_keep + 1));
    const int64_t b = r / (n_keep + 1);
    const int src = n == 0 ? 0 : min(max(keep[b * n_keep + n - 1], 0), np - 1) + 1;
    ((float4*)out)[i] = ((const float4*)pos)[(int64_t)src * d4 + c];
  }
}

// One mixed pixel of the patchify kernels' MIX variants (MixRow in kernels.h): fp32, contraction off
PVR_DEV float mix_value(float own, float par, bool inside, float lam, float oml) {
#pragma clang fp contract(off)
  return inside ? par : lam == 1.f ? own : lam * own + oml * par;
}

// mix[b] with the partner index made safe to use (the host validates the plan it was given; a device
// tensor that differs from it must still never index outside the batch)
PVR_DEV MixRow mix_row(const MixRow* __restrict__ mix, int b, int B) {
  const int4 lo = ((const int4*)(mix + b))[0], hi = ((const int4*)(mix + b))[1];
  MixRow r;
  r.partner = (unsigned)lo.x < (unsigned)B ? lo.x : b;
  r.lam = __int_as_float(lo.y);
  r.bx0 = lo.z; r.by0 = lo.w; r.bx1 = hi.x; r.by1 = hi.y;
  return r;
}

// a[c] of a by-value kernel argument without a divergent index into the argument segment
PVR_DEV float pick4(const float (&a)[4], int c) { return c == 0 ? a[0] : c == 1 ? a[1] : c == 2 ? a[2] : a[3]; }

// Random erasing (EraseRow / EraseArgs in kernels.h). The "pixel" fill of element e at site seed sd: a
// standard normal by Box-Muller from two hashes of the dropout counter. u1 = ((h1 >> 8) + 1) * 2^-24 lies
// in (0, 1] and u2 = (h2 >> 8) * 2^-24 in [0, 1), both exact in fp32, so |z| <= sqrt(2 * 24 * ln 2) = 5.77.
// fp32, contraction off, every operation rounded on its own. The patchify kernels and
// erase_noise_kernel call this one function, so the tests' host replay sees the kernels' bits.
PVR_DEV float erase_normal(uint64_t sd, uint64_t e) {
#pragma clang fp contract(off)
  const uint32_t h1 = rng_hash(sd, 2 * e), h2 = rng_hash(sd, 2 * e + 1);
  const float u1 = (float)((h1 >> 8) + 1u) * 5.9604644775390625e-08f;
  const float u2 = (float)(h2 >> 8) * 5.9604644775390625e-08f;
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831853f * u2);
}

// The fill of pixel (s, c, y, x) of a [.][C][H][W] model image (sd: *er.seed + er.offset in ERASE_PIXEL mode)
PVR_DEV float erase_fill(const EraseArgs& er, uint64_t sd, int s, int c, int y, int x, int C, int H, int W) {
  if (er.mode == ERASE_PIXEL) return erase_normal(sd, (((uint64_t)s * C + c) * H + y) * W + x);
  return pick4(er.value, c);
}

PVR_DEV bool erase_hit(const EraseRow& e, int x, int y) { return x >= e.x0 && x < e.x1 && y >= e.y0 && y < e.y1; }

PVR_DEV EraseRow erase_row(const EraseRow* __restrict__ rows, int b) {
  const int4 q = *(const int4*)(rows + b);
  return EraseRow{q.x, q.y, q.z, q.w};
}

// The mix row of an ERASE kernel: without a plan the identity (partner = self, lam == 1, empty box), under
// which mix_value selects the sample's own value and no partner pixel is read
PVR_DEV MixRow erase_mix_row(const MixRow* __restrict__ mix, int b, int B) {
  if (mix) return mix_row(mix, b, B);
  MixRow r;
  r.partner = b; r.lam = 1.f;
  r.bx0 = r.by0 = r.bx1 = r.by1 = 0;
  return r;
}

__global__ void __launch_bounds__(256) erase_noise_kernel(const uint64_t* seed_ptr, uint64_t off, float* __restrict__ out, int64_t n) {
  const uint64_t sd = *seed_ptr + off;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = erase_normal(sd, (uint64_t)i);
}

// img [B][C][H][W] fp32 -> patches [B*np][Kp] bf16, k = (c*P + ph)*P + pw, zero padded to Kp.
// One thread per 8 consecutive k of a patch row: with P % 8 == 0 they are 8 consecutive pixels of
// one image row (two float4 loads, one 16-B store); the zero padding past C*P*P and other patch
// sizes (P = 14) take the per-element path.
// MIX: sample b's pixels are blended with / replaced by those of sample mix[b].partner while they
// are gathered (mixup / CutMix, see MixRow in kernels.h). A pixel whose weight is 0 or 1 is read from
// one sample only, so CutMix moves the bytes of the plain gather; mixup reads the input twice.
// KEEP (patch dropout, both patchify kernels): only n_keep patches per sample are gathered. Output row r
// belongs to sample r / n_keep and holds patch keep[r] of it (keep [B][n_keep] int32, ascending per
// sample: patch_keep_kernel); the pixels, the padding and the mix plan (a box is in image pixels) are
// those of that patch in the plain kernel.
// ERASE (random erasing, both patchify kernels; only with MIX, whose plan may then be null = identity): a
// sample's own value inside its erase box er.rows[sample] is the fill (erase_fill) instead of the pixel,
// before the mix formula: the own and the partner pixel each test their own sample's box. An erased
// pixel is not loaded (eight erased pixels of the vector path load nothing); the loads that remain are
// those of the MIX kernel, inside the image. C <= 4 (the fill's per-channel value; host-checked).
// The fills of a thread's 8 pixels stay unrolled (16 call sites per code shape, 8 - 12 k instructions per
// instantiation): one rolled loop over the erased pixels is a third of the code but measured 10 % slower,
// a thread's fills then running one after the other (profiles/random_erasing/).
template <bool MIX, bool KEEP = false, bool ERASE = false>
__global__ void __launch_bounds__(256) im2col_kernel(const float* __restrict__ img, uint16_t* __restrict__ out,
                                                      int B, int C, int H, int W, int P, int Kp,
                                                      const MixRow* __restrict__ mix, const int* __restrict__ keep, int n_keep,
                                                      EraseArgs er) {
  static_assert(MIX || !ERASE, "ERASE exists only together with MIX");
  uint64_t esd = 0;
  if constexpr (ERASE) {
    if (er.mode == ERASE_PIXEL) esd = *er.seed + er.offset;
  }
  const int gw = W / P, np = (H / P) * gw;
  const int kc = C * P * P, k8 = Kp / 8;
  const bool vec = (P % 8 == 0) && (W % 4 == 0);
  const int64_t total = (int64_t)B * (KEEP ? n_keep : np) * k8;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k0 = (int)(i % k8) * 8;
    const int64_t rowi = i / k8;
    const int pidx = KEEP ? min(max(keep[rowi], 0), np - 1) : (int)(rowi % np);
    const int b = (int)(rowi / (KEEP ? n_keep : np));
    const int y0 = (pidx / gw) * P, x0 = (pidx % gw) * P;
    float v[8];
    if constexpr (MIX) {
      const MixRow r = ERASE ? erase_mix_row(mix, b, B) : mix_row(mix, b, B);
      const float oml = 1.0f - r.lam;
      EraseRow eo = {0, 0, 0, 0}, ep = eo;  // the own and the partner sample's erase box
      if constexpr (ERASE) {
        eo = erase_row(er.rows, b);
        ep = erase_row(er.rows, r.partner);
      }
      if (vec && k0 + 8 <= kc) {
        const int c = k0 / (P * P), rem = k0 % (P * P), ph = rem / P, pw = rem % P;
        const int y = y0 + ph, x = x0 + pw;
        const bool yin = y >= r.by0 && y < r.by1;
        bool in[8];
        int n_in = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          in[j] = yin && x + j >= r.bx0 && x + j < r.bx1;
          n_in += in[j];
        }
        const int64_t off = ((int64_t)c * H + y) * W + x;
        float4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, p0 = a0, p1 = a0;
        if constexpr (ERASE) {
          bool ea[8], eq[8], need_a = false, need_p = false;  // the own / the partner pixel is used and erased
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const bool use_p = in[j] || r.lam != 1.f;
            ea[j] = !in[j] && erase_hit(eo, x + j, y);
            eq[j] = use_p && erase_hit(ep, x + j, y);
            need_a |= !in[j] && !ea[j];
            need_p |= use_p && !eq[j];
          }
          if (need_a) {
            const float* src = img + (int64_t)b * C * H * W + off;
            a0 = *(const float4*)src; a1 = *(const float4*)(src + 4);
          }
          if (need_p) {
            const float* src = img + (int64_t)r.partner * C * H * W + off;
            p0 = *(const float4*)src; p1 = *(const float4*)(src + 4);
          }
          const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
          const float p[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float fa = ea[j] ? erase_fill(er, esd, b, c, y, x + j, C, H, W) : a[j];
            const float fp = eq[j] ? erase_fill(er, esd, r.partner, c, y, x + j, C, H, W) : p[j];
            v[j] = mix_value(fa, fp, in[j], r.lam, oml);
          }
        } else {
          if (n_in < 8) {
            const float* src = img + (int64_t)b * C * H * W + off;
            a0 = *(const float4*)src; a1 = *(const float4*)(src + 4);
          }
          if (n_in > 0 || r.lam != 1.f) {
            const float* src = img + (int64_t)r.partner * C * H * W + off;
            p0 = *(const float4*)src; p1 = *(const float4*)(src + 4);
          }
          const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
          const float p[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = mix_value(a[j], p[j], in[j], r.lam, oml);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = k0 + j;
          v[j] = 0.f;
          if (k < kc) {
            const int c = k / (P * P), rem = k % (P * P), ph = rem / P, pw = rem % P;
            const int y = y0 + ph, x = x0 + pw;
            const bool in = y >= r.by0 && y < r.by1 && x >= r.bx0 && x < r.bx1;
            const int64_t off = ((int64_t)c * H + y) * W + x;
            float a = 0.f, p = 0.f;
            if constexpr (ERASE) {
              if (!in) a = erase_hit(eo, x, y) ? erase_fill(er, esd, b, c, y, x, C, H, W) : img[(int64_t)b * C * H * W + off];
              if (in || r.lam != 1.f)
                p = erase_hit(ep, x, y) ? erase_fill(er, esd, r.partner, c, y, x, C, H, W) : img[(int64_t)r.partner * C * H * W + off];
            } else {
              if (!in) a = img[(int64_t)b * C * H * W + off];
              if (in || r.lam != 1.f) p = img[(int64_t)r.partner * C * H * W + off];
            }
            v[j] = mix_value(a, p, in, r.lam, oml);
          }
        }
      }
    } else if (vec && k0 + 8 <= kc) {
      const int c = k0 / (P * P), rem = k0 % (P * P), ph = rem / P, pw = rem % P;
      const float* src = img + (((int64_t)b * C + c) * H + y0 + ph) * W + x0 + pw;
      const float4 a = *(const float4*)src, bq = *(const float4*)(src + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = bq.x; v[5] = bq.y; v[6] = bq.z; v[7] = bq.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        v[j] = 0.f;
        if (k < kc) {
          const int c = k / (P * P), rem = k % (P * P), ph = rem / P, pw = rem % P;
          v[j] = img[(((int64_t)b * C + c) * H + y0 + ph) * W + x0 + pw];
        }
      }
    }
    uint4 o;
    o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]); o.z = pack2bf(v[4], v[5]); o.w = pack2bf(v[6], v[7]);
    *(uint4*)(out + rowi * Kp + k0) = o;
  }
}

// uint8 source image -> the same bf16 patch rows as im2col_kernel, with the input pipeline's
// per-image work fused in: scale to [0,1], per-channel normalise and (GEOM) a per-sample crop box
// resampled bilinearly to H x W, flipped when the box runs right to left.
//   img  [B][C <= 4][Hs][Ws] uint8 by element strides (sb, sc, sy, sx): contiguous NCHW and
//        channels_last are both read in place
//   geom [B][4] = (x0, y0, x1, y1) in source pixel-edge coordinates, x0 > x1 = flipped
// All arithmetic is fp32 in the order of the PyTorch reference (data/device_input.py
// preprocess_reference), every operation rounded on its own: contraction is off in this
// kernel, and the two divisions of ((p / 255) - mean) / std are correctly rounded (hipcc's default;
// a multiply by 1/255 differs from the division in the last bit for 126 of the 256 byte values).
// Without GEOM (Hs == H, Ws == W) and with `vec` (host-checked: sx == 1, P % 8 == 0, base and every
// other stride 8-byte aligned) the 8 pixels of a thread are one 8-byte load; otherwise per element.
struct U8Norm {
  float mean[4], stdv[4];
};

PVR_DEV float u8_normalise(float p, float mean, float stdv) {
#pragma clang fp contract(off)
  return (p / 255.0f - mean) / stdv;
}

// Source coordinate of output index o along one axis: box start e0, step = (e1 - e0) / n_out;
// returns the two taps i <= j (both inside [0, n_src - 1] for any e0 / step, NaN included) and the weight of j.
PVR_DEV void u8_axis(int o, float e0, float step, int n_src, int& i, int& j, float& w) {
#pragma clang fp contract(off)
  float s = e0 + ((float)o + 0.5f) * step - 0.5f;
  s = fminf(fmaxf(s, 0.f), (float)(n_src - 1));  // fmaxf(NaN, 0) = 0
  const float f = floorf(s);
  i = min(max((int)f, 0), n_src - 1);
  j = min(i + 1, n_src - 1);
  w = s - f;
}

// Output pixel (x, y) of one channel plane under crop box g (steps precomputed): the bilinear sample
// of the four taps, normalised; fp32, before the bf16 cast. The GEOM loop body of im2col_u8_kernel as
// a function, for its MIX variant, which samples two images per pixel (the no-mix kernel keeps the
// body inline: calling this there schedules differently).
PVR_DEV float u8_sample(const uint8_t* src_c, int64_t sy, int64_t sx, const float4& g, float stepx, float stepy, int x, int y,
                        int Ws, int Hs, float mean, float stdv) {
#pragma clang fp contract(off)
  int xi, xj, yi, yj;
  float wx, wy;
  u8_axis(x, g.x, stepx, Ws, xi, xj, wx);
  u8_axis(y, g.y, stepy, Hs, yi, yj, wy);
  const float ta = (float)src_c[yi * sy + xi * sx], tb = (float)src_c[yi * sy + xj * sx];
  const float tc = (float)src_c[yj * sy + xi * sx], td = (float)src_c[yj * sy + xj * sx];
  const float top = ta + wx * (tb - ta), bot = tc + wx * (td - tc);
  return u8_normalise(top + wy * (bot - top), mean, stdv);
}

// MIX (see im2col_kernel): the blend runs on the normalised fp32 values, each sample under its own
// crop box, so the no-GEOM table then holds fp32 values instead of their bf16 roundings.
// KEEP: as in im2col_kernel.
// ERASE: as in im2col_kernel; the fill replaces the normalised value.
template <bool GEOM, bool MIX, bool KEEP = false, bool ERASE = false>
__global__ void __launch_bounds__(256) im2col_u8_kernel(const uint8_t* __restrict__ img, int64_t sb, int64_t sc, int64_t sy,
                                                         int64_t sx, U8Norm nrm, const float* __restrict__ geom,
                                                         uint16_t* __restrict__ out, int B, int C, int Hs, int Ws, int H, int W,
                                                         int P, int Kp, int vec, const MixRow* __restrict__ mix,
                                                         const int* __restrict__ keep, int n_keep, EraseArgs er) {
#pragma clang fp contract(off)
  static_assert(MIX || !ERASE, "ERASE exists only together with MIX");
  uint64_t esd = 0;
  if constexpr (ERASE) {
    if (er.mode == ERASE_PIXEL) esd = *er.seed + er.offset;
  }
  // Without GEOM a pixel is one of 256 byte values: each block tabulates the normalised bf16 of every
  // (channel, byte) pair once, with the same operations and hence the same bits, and its loop does
  // no division. Two correctly rounded divisions per element make the kernel ALU-bound: 51 us
  // against 38 us with the table at 256 x 224 x 224 (the float kernel: 43 us), profiles/input_u8/.
  __shared__ uint16_t lut[GEOM || MIX ? 1 : 4][256];
  __shared__ float lutf[!GEOM && MIX ? 4 : 1][256];
  if constexpr (!GEOM && MIX) {
    for (int c = 0; c < C; ++c) lutf[c][threadIdx.x] = u8_normalise((float)threadIdx.x, nrm.mean[c], nrm.stdv[c]);
    __syncthreads();
  } else if constexpr (!GEOM) {
    for (int c = 0; c < C; ++c) lut[c][threadIdx.x] = f2bf(u8_normalise((float)threadIdx.x, nrm.mean[c], nrm.stdv[c]));
    __syncthreads();
  }
  const int gw = W / P, np = (H / P) * gw;
  const int kc = C * P * P, k8 = Kp / 8;
  const int64_t total = (int64_t)B * (KEEP ? n_keep : np) * k8;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k0 = (int)(i % k8) * 8;
    const int64_t rowi = i / k8;
    const int pidx = KEEP ? min(max(keep[rowi], 0), np - 1) : (int)(rowi % np);
    const int b = (int)(rowi / (KEEP ? n_keep : np));
    const int py = (pidx / gw) * P, px = (pidx % gw) * P;
    const uint8_t* src_b = img + b * sb;
    uint32_t h[8];  // bf16 bits
    if constexpr (MIX) {
      const MixRow r = ERASE ? erase_mix_row(mix, b, B) : mix_row(mix, b, B);
      const float oml = 1.0f - r.lam;
      const uint8_t* src_p = img + r.partner * sb;
      float v[8];
      EraseRow eo = {0, 0, 0, 0}, ep = eo;  // the own and the partner sample's erase box
      if constexpr (ERASE) {
        eo = erase_row(er.rows, b);
        ep = erase_row(er.rows, r.partner);
      }
      if constexpr (!GEOM) {
        if (vec && k0 + 8 <= kc) {
          const int c = k0 / (P * P), rem = k0 % (P * P), ph = rem / P, pw = rem % P;
          const int y = py + ph, x = px + pw;
          const bool yin = y >= r.by0 && y < r.by1;
          bool in[8];
          int n_in = 0;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            in[j] = yin && x + j >= r.bx0 && x + j < r.bx1;
            n_in += in[j];
          }
          const int64_t off = c * sc + (int64_t)y * sy + x;
          uint2 qa = {0u, 0u}, qp = {0u, 0u};
          if constexpr (ERASE) {
            bool ea[8], eq[8], need_a = false, need_p = false;  // the own / the partner pixel is used and erased
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const bool use_p = in[j] || r.lam != 1.f;
              ea[j] = !in[j] && erase_hit(eo, x + j, y);
              eq[j] = use_p && erase_hit(ep, x + j, y);
              need_a |= !in[j] && !ea[j];
              need_p |= use_p && !eq[j];
            }
            if (need_a) qa = *(const uint2*)(src_b + off);
            if (need_p) qp = *(const uint2*)(src_p + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const uint32_t a = ((j < 4 ? qa.x : qa.y) >> (8 * (j & 3))) & 0xFFu;
              const uint32_t p = ((j < 4 ? qp.x : qp.y) >> (8 * (j & 3))) & 0xFFu;
              const float fa = ea[j] ? erase_fill(er, esd, b, c, y, x + j, C, H, W) : lutf[c][a];
              const float fp = eq[j] ? erase_fill(er, esd, r.partner, c, y, x + j, C, H, W) : lutf[c][p];
              v[j] = mix_value(fa, fp, in[j], r.lam, oml);
            }
          } else {
            if (n_in < 8) qa = *(const uint2*)(src_b + off);
            if (n_in > 0 || r.lam != 1.f) qp = *(const uint2*)(src_p + off);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const uint32_t a = ((j < 4 ? qa.x : qa.y) >> (8 * (j & 3))) & 0xFFu;
              const uint32_t p = ((j < 4 ? qp.x : qp.y) >> (8 * (j & 3))) & 0xFFu;
              v[j] = mix_value(lutf[c][a], lutf[c][p], in[j], r.lam, oml);
            }
          }
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int k = k0 + j;
            v[j] = 0.f;
            if (k < kc) {
              const int c = k / (P * P), rem = k % (P * P), ph = rem / P, pw = rem % P;
              const int y = py + ph, x = px + pw;
              const bool in = y >= r.by0 && y < r.by1 && x >= r.bx0 && x < r.bx1;
              const int64_t off = c * sc + (int64_t)y * sy + (int64_t)x * sx;
              float a = 0.f, p = 0.f;
              if constexpr (ERASE) {
                if (!in) a = erase_hit(eo, x, y) ? erase_fill(er, esd, b, c, y, x, C, H, W) : lutf[c][src_b[off]];
                if (in || r.lam != 1.f) p = erase_hit(ep, x, y) ? erase_fill(er, esd, r.partner, c, y, x, C, H, W) : lutf[c][src_p[off]];
              } else {
                if (!in) a = lutf[c][src_b[off]];
                if (in || r.lam != 1.f) p = lutf[c][src_p[off]];
              }
              v[j] = mix_value(a, p, in, r.lam, oml);
            }
          }
        }
      } else {
        // each sample under its own crop box
        const float4 g = *(const float4*)(geom + (int64_t)b * 4), gp = *(const float4*)(geom + (int64_t)r.partner * 4);
        const float stepx = (g.z - g.x) / (float)W, stepy = (g.w - g.y) / (float)H;
        const float pstepx = (gp.z - gp.x) / (float)W, pstepy = (gp.w - gp.y) / (float)H;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = k0 + j;
          v[j] = 0.f;
          if (k < kc) {
            const int c = k / (P * P), rem = k % (P * P), ph = rem / P, pw = rem % P;
            const int y = py + ph, x = px + pw;
            const bool in = y >= r.by0 && y < r.by1 && x >= r.bx0 && x < r.bx1;
            const float mean = pick4(nrm.mean, c), stdv = pick4(nrm.stdv, c);
            float a = 0.f, p = 0.f;
            if constexpr (ERASE) {
              if (!in)
                a = erase_hit(eo, x, y) ? erase_fill(er, esd, b, c, y, x, C, H, W)
                                        : u8_sample(src_b + c * sc, sy, sx, g, stepx, stepy, x, y, Ws, Hs, mean, stdv);
              if (in || r.lam != 1.f)
                p = erase_hit(ep, x, y) ? erase_fill(er, esd, r.partner, c, y, x, C, H, W)
                                        : u8_sample(src_p + c * sc, sy, sx, gp, pstepx, pstepy, x, y, Ws, Hs, mean, stdv);
            } else {
              if (!in) a = u8_sample(src_b + c * sc, sy, sx, g, stepx, stepy, x, y, Ws, Hs, mean, stdv);
              if (in || r.lam != 1.f) p = u8_sample(src_p + c * sc, sy, sx, gp, pstepx, pstepy, x, y, Ws, Hs, mean, stdv);
            }
            v[j] = mix_value(a, p, in, r.lam, oml);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = f2bf(v[j]);
    } else if constexpr (!GEOM) {
      if (vec && k0 + 8 <= kc) {
        const int c = k0 / (P * P), rem = k0 % (P * P), ph = rem / P, pw = rem % P;
        const uint2 q = *(const uint2*)(src_b + c * sc + (int64_t)(py + ph) * sy + px + pw);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          h[j] = lut[c][(q.x >> (8 * j)) & 0xFFu];
          h[4 + j] = lut[c][(q.y >> (8 * j)) & 0xFFu];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = k0 + j;
          h[j] = 0;
          if (k < kc) {
            const int c = k / (P * P), rem = k % (P * P), ph = rem / P, pw = rem % P;
            h[j] = lut[c][src_b[c * sc + (int64_t)(py + ph) * sy + (int64_t)(px + pw) * sx]];
          }
        }
      }
    } else {
      const float4 g = *(const float4*)(geom + (int64_t)b * 4);
      const float stepx = (g.z - g.x) / (float)W, stepy = (g.w - g.y) / (float)H;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        h[j] = 0;
        if (k < kc) {
          const int c = k / (P * P), rem = k % (P * P), ph = rem / P, pw = rem % P;
          const uint8_t* src_c = src_b + c * sc;
          int xi, xj, yi, yj;
          float wx, wy;
          u8_axis(px + pw, g.x, stepx, Ws, xi, xj, wx);
          u8_axis(py + ph, g.y, stepy, Hs, yi, yj, wy);
          const float ta = (float)src_c[yi * sy + xi * sx], tb = (float)src_c[yi * sy + xj * sx];
          const float tc = (float)src_c[yj * sy + xi * sx], td = (float)src_c[yj * sy + xj * sx];
          const float top = ta + wx * (tb - ta), bot = tc + wx * (td - tc);
          h[j] = f2bf(u8_normalise(top + wy * (bot - top), pick4(nrm.mean, c), pick4(nrm.stdv, c)));
        }
      }
    }
    uint4 o;
    o.x = h[0] | (h[1] << 16); o.y = h[2] | (h[3] << 16); o.z = h[4] | (h[5] << 16); o.w = h[6] | (h[7] << 16);
    *(uint4*)(out + rowi * Kp + k0) = o;
  }
}

// out[b][0][:] = dropout(cls + pos[0])   (row b*(np+1) of the token tensor)
__global__ void __launch_bounds__(256) cls_rows_kernel(const float* __restrict__ cls, const float* __restrict__ pos,
                                                        uint16_t* __restrict__ out, int B, int D, int64_t row_stride,
                                                        const uint64_t* seed_ptr, uint64_t seed_off, uint32_t thr, float scale,
                                                        int64_t ncols_total) {
  const uint64_t seed = thr ? (*seed_ptr + seed_off) : 0ull;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < B * D; i += gridDim.x * 256) {
    const int b = i / D, d = i % D;
    float v = cls[d] + pos[d];
    // dropout index uses the logical [B*(np+1), D] element index (row b*(np+1))
    if (thr) v = rng_keep(seed, (uint64_t)(b * (row_stride / D)) * D + d, thr) ? v * scale : 0.f;
    out[(int64_t)b * row_stride + d] = f2bf(v);
  }
}

// Backward of  E = dropout(concat(cls, conv) + pos):  dE [B][np+1][D] bf16 ->
//   dpre = dE * mask;  dpos[n][d] += sum_b dpre;  dcls[d] += sum_b dpre[b][0][d];
//   dconv[b*np + n-1][d] = dpre (bf16, n >= 1);  dbias[d] += sum_{b, n>=1} dpre.
// Two passes and (almost) no atomics: device-scope f32 atomics that pile onto a few KB of addresses
// (dbias: 768 columns) serialise. At ViT-B/16 b256 this is 33 us; the one-pass kernel that added
// per-block partials with atomics took 250 us, one adding per-thread partials ~450 us
// (scripts/atomics_probe.py, profiles/atomics_probe.log).
//  pass 1: thread = one (token, 8-column chunk) pair of the flattened [ntok][D/8] grid (every lane
//          busy; D/8 = 96 does not fill power-of-two blocks), block.y = a group of PB_BAT images;
//          8 independent 16-B loads in flight per thread; writes the masked gradient (dconv) and
//          the group's per-(token, column) sums to ws[group][ntok][D] with plain stores;
//  pass 2: thread = (8-column chunk, token) sums the groups, owns dpos[n] (and dcls for n = 0), and
//          the block reduces its tokens' dbias partials in LDS into one partial row per token block;
//  pass 3: the conv-bias gradient sums those rows in block order (deterministic, no atomics).
// KEEP (patch dropout): dE is the compact [B][n_keep + 1][D] token gradient and inv [B][ntok - 1] gives the
// compact slot of each patch (-1: dropped, patch_keep_kernel). The thread still owns position n of the
// full sequence: for image b it reads compact row 1 + inv[b][n - 1] (row 0 for n = 0), masks it at that
// compact element index (the forward's) and stores it to dconv [B * n_keep][D]; a dropped patch is
// skipped, so a position no image of the group kept sums to exact zeros. ws / passes 2 and 3 are unchanged.
constexpr int PB_BAT = 32, PB_UNROLL = 8;
template <bool KEEP>
__global__ void __launch_bounds__(256) patch_bwd_kernel(const uint16_t* __restrict__ dE, int B, int ntok, int D,
                                                         float* __restrict__ ws, uint16_t* __restrict__ dconv,
                                                         const uint64_t* seed_ptr, uint64_t seed_off, uint32_t thr, float scale,
                                                         const int* __restrict__ inv, int n_keep) {
  const uint64_t seed = thr ? (*seed_ptr + seed_off) : 0ull;
  const int nch = D >> 3;
  const int flat = blockIdx.x * 256 + threadIdx.x;
  if (flat >= ntok * nch) return;
  const int n = flat / nch, c = flat - n * nch;
  const int b0 = blockIdx.y * PB_BAT, b1 = min(B, b0 + PB_BAT);
  const int rows_img = KEEP ? n_keep + 1 : ntok;          // token rows of one image in dE
  const int64_t img_stride = (int64_t)rows_img * D;       // elements between consecutive images
  const uint16_t* src = dE + (KEEP ? 0 : (int64_t)n * D) + c * 8;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int bb = b0; bb < b1; bb += PB_UNROLL) {
    uint4 q[PB_UNROLL];
    int row[PB_UNROLL];  // KEEP: the compact row of position n in image bb + u, -1: dropped
    if constexpr (KEEP) {
#pragma unroll
      for (int u = 0; u < PB_UNROLL; ++u) {
        row[u] = 0;
        if (n > 0) {
          const int sl = inv[(int64_t)min(bb + u, b1 - 1) * (ntok - 1) + n - 1];
          row[u] = (sl >= 0 && sl < n_keep) ? sl + 1 : -1;
        }
      }
#pragma unroll
      for (int u = 0; u < PB_UNROLL; ++u) {
        q[u] = make_uint4(0u, 0u, 0u, 0u);
        if (row[u] >= 0) q[u] = *(const uint4*)(src + (int64_t)min(bb + u, b1 - 1) * img_stride + (int64_t)row[u] * D);
      }
    } else {
#pragma unroll
      for (int u = 0; u < PB_UNROLL; ++u) q[u] = *(const uint4*)(src + (int64_t)min(bb + u, b1 - 1) * img_stride);
    }
#pragma unroll
    for (int u = 0; u < PB_UNROLL; ++u) {
      const int b = bb + u;
      if (b >= b1) break;
      if constexpr (KEEP) {
        if (row[u] < 0) continue;
      }
      const int tok = KEEP ? row[u] : n;  // the row's token index inside its image
      const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
      float v[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[2 * j] = bf2f(w[j] & 0xFFFF);
        v[2 * j + 1] = bf2f(w[j] >> 16);
      }
      if (thr) {
        const uint64_t e0 = ((uint64_t)b * rows_img + tok) * D + c * 8;
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          bool k0, k1;
          rng_keep2(seed, e0 + j, thr, k0, k1);
          v[j] = k0 ? v[j] * scale : 0.f;
          v[j + 1] = k1 ? v[j + 1] * scale : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] += v[j];
      if (n > 0 && dconv) {
        uint4 o;
        o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]); o.z = pack2bf(v[4], v[5]); o.w = pack2bf(v[6], v[7]);
        *(uint4*)(dconv + ((int64_t)b * (rows_img - 1) + tok - 1) * D + c * 8) = o;
      }
    }
  }
  float* o = ws + ((int64_t)blockIdx.y * ntok + n) * D + c * 8;
  *(float4*)o = make_float4(s[0], s[1], s[2], s[3]);
  *(float4*)(o + 4) = make_float4(s[4], s[5], s[6], s[7]);
}

constexpr int PR_CH = 32, PR_TOK = 8;  // pass-2 block: 32 column chunks x 8 tokens
__global__ void __launch_bounds__(256) patch_bwd_reduce_kernel(const float* __restrict__ ws, int G, int ntok, int D,
                                                                float* __restrict__ dpos, float* __restrict__ dcls,
                                                                float* __restrict__ dbias_part) {
  __shared__ float red[PR_TOK][PR_CH * 8];
  const int nch = D >> 3;
  const int cl = threadIdx.x % PR_CH, tl = threadIdx.x / PR_CH;
  const int c = blockIdx.x * PR_CH + cl;
  const int n = blockIdx.y * PR_TOK + tl;
  float t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool ok = c < nch && n < ntok;
  if (ok) {
    const float* src = ws + (int64_t)n * D + c * 8;
    const int64_t gs = (int64_t)ntok * D;
    int g = 0;
    for (; g + 4 <= G; g += 4) {
      float4 a[8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a[2 * u] = *(const float4*)(src + (g + u) * gs);
        a[2 * u + 1] = *(const float4*)(src + (g + u) * gs + 4);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        t[0] += a[2 * u].x; t[1] += a[2 * u].y; t[2] += a[2 * u].z; t[3] += a[2 * u].w;
        t[4] += a[2 * u + 1].x; t[5] += a[2 * u + 1].y; t[6] += a[2 * u + 1].z; t[7] += a[2 * u + 1].w;
      }
    }
    for (; g < G; ++g) {
      const float4 a0 = *(const float4*)(src + g * gs), a1 = *(const float4*)(src + g * gs + 4);
      t[0] += a0.x; t[1] += a0.y; t[2] += a0.z; t[3] += a0.w;
      t[4] += a1.x; t[5] += a1.y; t[6] += a1.z; t[7] += a1.w;
    }
    if (dpos) {  // this thread owns dpos[n][c*8 .. +8]
      float* d = dpos + (int64_t)n * D + c * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] += t[j];
    }
    if (n == 0 && dcls) {
#pragma unroll
      for (int j = 0; j < 8; ++j) dcls[c * 8 + j] += t[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[tl][cl * 8 + j] = (ok && n > 0) ? t[j] : 0.f;
  __syncthreads();
  if (dbias_part) {  // this token block's partial column sums (summed in block order below: deterministic)
    const int col = blockIdx.x * PR_CH * 8 + threadIdx.x;  // 256 columns per block, one per thread
    if (col < D) {
      float a = 0.f;
#pragma unroll
      for (int k = 0; k < PR_TOK; ++k) a += red[k][threadIdx.x];
      dbias_part[(int64_t)blockIdx.y * D + col] = a;
    }
  }
}

// Deterministic column reduction of partial rows: dst[c] += sum_r part[r][c] in row order, the C
// columns split into segments of `seg` going to d0 / d1 / d2 (null: dropped). Block = 8 row lanes x
// 32 columns; lane rl sums rows rl, rl + 8, ... and the 8 lane sums are added in lane order: the same
// bits on every run (the float-atomic reductions it replaces are order-dependent).
__global__ void __launch_bounds__(256) rows_reduce_kernel(const float* __restrict__ part, int R, int C, int seg,
                                                           float* __restrict__ d0, float* __restrict__ d1, float* __restrict__ d2) {
  __shared__ float red[8][33];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c = blockIdx.x * 32 + cl;
  float a = 0.f;
  if (c < C) {
    int r = rl;
    for (; r + 24 < R; r += 32) {  // four independent loads in flight
      const float x0 = part[(int64_t)r * C + c], x1 = part[(int64_t)(r + 8) * C + c];
      const float x2 = part[(int64_t)(r + 16) * C + c], x3 = part[(int64_t)(r + 24) * C + c];
      a += x0; a += x1; a += x2; a += x3;
    }
    for (; r < R; r += 8) a += part[(int64_t)r * C + c];
  }
  red[rl][cl] = a;
  __syncthreads();
  if (rl == 0 && c < C) {
    float t = red[0][cl];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += red[k][cl];
    float* d = c < seg ? d0 : (c < 2 * seg ? d1 : d2);
    if (d) d[c % seg] += t;
  }
}

// Batched bf16 transpose: matrix t (rows R_t, cols C_t) at src + soff[t] -> dst + doff[t] as [C_t][R_t].
// 64x64 tiles through LDS held as bf16 pairs (u32, 33-word rows: conflict-free column reads);
// 16-B loads and stores, 8 lanes per 128-B row. tile_start[t] = prefix tile count (binary search).
__global__ void __launch_bounds__(256) transpose_batched_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst,
                                                                 const int64_t* __restrict__ meta, int nmat) {
  __shared__ uint32_t tile[64][33];
  const int blk = blockIdx.x;
  int lo = 0, hi = nmat - 1;  // last t with tile_start[t] <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (meta[mid * 5 + 4] <= blk) lo = mid; else hi = mid - 1;
  }
  const int t = lo;
  const int64_t soff = meta[t * 5 + 0], doff = meta[t * 5 + 1];
  const int R = (int)meta[t * 5 + 2], C = (int)meta[t * 5 + 3];
  const int local = blk - (int)meta[t * 5 + 4];
  const int tc = (C + 63) / 64;
  const int r0 = (local / tc) * 64, c0 = (local % tc) * 64;
  const bool full = r0 + 64 <= R && c0 + 64 <= C && (C % 8) == 0 && (R % 8) == 0 && (soff % 8) == 0 && (doff % 8) == 0;
  const int tid = threadIdx.x;
  if (full) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int row = tid / 8 + 32 * it, ch = tid % 8;
      const uint4 q = *(const uint4*)(src + soff + (int64_t)(r0 + row) * C + c0 + ch * 8);
      tile[row][ch * 4 + 0] = q.x; tile[row][ch * 4 + 1] = q.y;
      tile[row][ch * 4 + 2] = q.z; tile[row][ch * 4 + 3] = q.w;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + 256 * it;
      const int cc = idx / 8, rch = idx % 8;  // output row (input column) cc, input rows rch*8 .. +7
      uint32_t h[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] = (tile[rch * 8 + j][cc >> 1] >> ((cc & 1) * 16)) & 0xFFFFu;
      uint4 o;
      o.x = h[0] | (h[1] << 16); o.y = h[2] | (h[3] << 16); o.z = h[4] | (h[5] << 16); o.w = h[6] | (h[7] << 16);
      *(uint4*)(dst + doff + (int64_t)(c0 + cc) * R + r0 + rch * 8) = o;
    }
    return;
  }
  uint16_t* t16 = (uint16_t*)&tile[0][0];  // edge tiles: element-wise through [64][66] bf16
  for (int i = tid; i < 64 * 64; i += 256) {
    const int rr = i / 64, cc = i % 64;
    if (r0 + rr < R && c0 + cc < C) t16[rr * 66 + cc] = src[soff + (int64_t)(r0 + rr) * C + c0 + cc];
  }
  __syncthreads();
  for (int i = tid; i < 64 * 64; i += 256) {
    const int cc = i / 64, rr = i % 64;
    if (r0 + rr < R && c0 + cc < C) dst[doff + (int64_t)(c0 + cc) * R + r0 + rr] = t16[rr * 66 + cc];
  }
}

// out (+)= sum over S split-K partial slices ws[s] (the second half of the store-then-reduce wgrad,
// tile 14); fixed slice order, so the result is deterministic. ws rows hold wcols floats, out rows
// the first ocols of them (ocols <= wcols, both % 4 == 0): a GEMM over a K padded to the tile width
// reduces straight into the unpadded weight gradient.
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* __restrict__ ws, int S, int64_t stride,
                                                            float* __restrict__ out, int64_t n4, int ocols, int wcols,
                                                            int accumulate) {
  const int oc4 = ocols / 4;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 a = accumulate ? ((const float4*)out)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t row = i / oc4;
    const float* src = ws + row * wcols + 4 * (i - row * oc4);
    int s = 0;
    for (; s + 4 <= S; s += 4) {  // 4 independent loads in flight per trip
      const float4 b0 = *(const float4*)(src + (int64_t)s * stride);
      const float4 b1 = *(const float4*)(src + (int64_t)(s + 1) * stride);
      const float4 b2 = *(const float4*)(src + (int64_t)(s + 2) * stride);
      const float4 b3 = *(const float4*)(src + (int64_t)(s + 3) * stride);
      a.x += (b0.x + b1.x) + (b2.x + b3.x);
      a.y += (b0.y + b1.y) + (b2.y + b3.y);
      a.z += (b0.z + b1.z) + (b2.z + b3.z);
      a.w += (b0.w + b1.w) + (b2.w + b3.w);
    }
    for (; s < S; ++s) {
      const float4 b = *(const float4*)(src + (int64_t)s * stride);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    ((float4*)out)[i] = a;
  }
}

// dst[r][c] = c < cols ? src[r][c] : 0 for c < ld_dst (bf16; cols, ld_dst % 4 == 0): the patch
// embedding's conv weight [D][C*P*P] zero-padded to the GEMM's K tile
__global__ void __launch_bounds__(256) pad_cols_bf16_kernel(const uint16_t* __restrict__ src, int rows, int cols,
                                                            uint16_t* __restrict__ dst, int ld_dst) {
  const int q = ld_dst / 4;
  const int64_t n4 = (int64_t)rows * q;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / q;
    const int c = 4 * (int)(i - r * q);
    uint2 v = make_uint2(0u, 0u);
    if (c < cols) v = *(const uint2*)(src + r * cols + c);
    *(uint2*)(dst + r * ld_dst + c) = v;
  }
}

}  // namespace
}  // namespace pvr

extern "C" hipError_t pvr_splitk_reduce(const float* ws, int S, int64_t stride, float* out, int64_t n, int ocols, int wcols,
                                        int accumulate, hipStream_t s) {
  using namespace pvr;
  if (n <= 0) return hipSuccess;
  if (n % 4 || stride % 4 || ocols <= 0 || ocols % 4 || wcols % 4 || ocols > wcols || n % ocols) return hipErrorInvalidValue;
  int64_t blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ws, S, stride, out, n / 4, ocols, wcols,
                     accumulate);
  return hipGetLastError();
}

extern "C" hipError_t pvr_pad_cols_bf16(const uint16_t* src, int rows, int cols, uint16_t* dst, int ld_dst, hipStream_t s) {
  using namespace pvr;
  if (rows <= 0) return hipSuccess;
  if (cols % 4 || ld_dst % 4 || cols > ld_dst) return hipErrorInvalidValue;
  int64_t blocks = ((int64_t)rows * (ld_dst / 4) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(pad_cols_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, rows, cols, dst, ld_dst);
  return hipGetLastError();
}

extern "C" hipError_t pvr_transpose_batched(const uint16_t* src, uint16_t* dst, const int64_t* meta, int nmat, int total_tiles,
                                            hipStream_t s) {
  using namespace pvr;
  if (total_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(transpose_batched_kernel, dim3(total_tiles), dim3(256), 0, s, src, dst, meta, nmat);
  return hipGetLastError();
}

extern "C" hipError_t pvr_cast_f32_bf16(const float* in, uint16_t* out, int64_t n, hipStream_t s) {
  using namespace pvr;
  if (n <= 0) return hipSuccess;
  int64_t blocks = (n / 4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, in, out, n);
  return hipGetLastError();
}

extern "C" int pvr_colsum_part_rows(int rows) {
  const int gy = (rows + 63) / 64;
  return gy > 256 ? 256 : gy;
}

extern "C" hipError_t pvr_colsum(const uint16_t* dy, int64_t ld, int rows, int N, float* db, uint16_t* dz, int64_t ld_dz,
                                 pvr::DropSite drop, pvr::Fp8Copy q, float* part, int row_mul, pvr::DropSite dpath, int dp_rows,
                                 hipStream_t s) {
  using namespace pvr;
  if (rows <= 0) return hipSuccess;
  if (row_mul < 1 || (int64_t)rows * row_mul >= (1ll << 31)) return hipErrorInvalidValue;
  if (N % 8 != 0 || (q.fmt != 0 && q.fmt != 1)) return hipErrorInvalidValue;
  if (q.out && (!q.scale || !q.amax || q.ld % 8 != 0 || reinterpret_cast<uintptr_t>(q.out) % 8 != 0)) return hipErrorInvalidValue;
  const bool has_dp = dpath.seed && dpath.thr;
  if (has_dp && (q.out || dp_rows < 1 || dpath.thr > 65535u)) return hipErrorInvalidValue;  // drop path: bf16 only
  const int gx = (N / 8 + 63) / 64;
  const int gy = pvr_colsum_part_rows(rows);
  if (!db) part = nullptr;
  hipLaunchKernelGGL(q.out ? colsum_kernel<true> : has_dp ? (colsum_kernel<false, true>) : colsum_kernel<false>, dim3(gx, gy), dim3(256), 0,
                     s, dy, ld, rows, N, db, dz, ld_dz, drop.seed, drop.offset, drop.thr, drop.scale, q.out, q.ld, q.scale, q.amax, q.fmt,
                     part, row_mul, dpath.seed, dpath.offset, has_dp ? dpath.thr : 0u, dpath.scale, dp_rows);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !part) return e;
  return pvr_rows_reduce(part, gy, N, N, db, nullptr, nullptr, s);
}

extern "C" hipError_t pvr_drop_path_scale(pvr::DropSite dpath, float* s_out, int B, hipStream_t s) {
  using namespace pvr;
  if (B <= 0) return hipSuccess;
  if (!dpath.seed || !s_out || dpath.thr > 65535u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(drop_path_scale_kernel, dim3((B + 255) / 256), dim3(256), 0, s, dpath.seed, dpath.offset, dpath.thr, dpath.scale,
                     s_out, B);
  return hipGetLastError();
}

extern "C" hipError_t pvr_patch_keep(const uint64_t* seed, uint64_t offset, int B, int np, int n_keep, int* keep, int* inv,
                                     hipStream_t s) {
  using namespace pvr;
  if (!seed || !keep || !inv || np < 1 || np > PK_MAX || n_keep < 1 || n_keep > np || B < 0 || (int64_t)B * np >= (1ll << 32))
    return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  hipLaunchKernelGGL(patch_keep_kernel, dim3(B), dim3(256), 0, s, seed, offset, np, n_keep, keep, inv);
  return hipGetLastError();
}

extern "C" hipError_t pvr_pos_gather(const float* pos, const int* keep, float* out, int B, int np, int n_keep, int D, hipStream_t s) {
  using namespace pvr;
  if (!pos || !keep || !out || np < 1 || n_keep < 1 || n_keep > np || D < 4 || D % 4 || reinterpret_cast<uintptr_t>(pos) % 16 ||
      reinterpret_cast<uintptr_t>(out) % 16)
    return hipErrorInvalidValue;
  const int64_t total = (int64_t)B * (n_keep + 1) * (D / 4);
  if (total <= 0) return hipSuccess;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pos_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pos, keep, out, B, np, n_keep, D);
  return hipGetLastError();
}

// an erase argument the kernels can take: an aligned table, a known mode, a seed in pixel mode, C <= 4
static bool erase_args_ok(const pvr::EraseArgs& e, int C) {
  if (!e.rows) return true;
  if (reinterpret_cast<uintptr_t>(e.rows) % 16 || C < 1 || C > 4) return false;
  return e.mode == pvr::ERASE_CONST || (e.mode == pvr::ERASE_PIXEL && e.seed);
}

extern "C" hipError_t pvr_erase_noise(const uint64_t* seed, uint64_t offset, float* out, int64_t n, hipStream_t s) {
  using namespace pvr;
  if (!seed || !out || n < 0) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(erase_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, s, seed, offset, out, n);
  return hipGetLastError();
}

extern "C" hipError_t pvr_im2col(const float* img, uint16_t* out, int B, int C, int H, int W, int P, int Kp,
                                 const pvr::MixRow* mix, const int* keep, int n_keep, pvr::EraseArgs erase, hipStream_t s) {
  using namespace pvr;
  if (Kp % 8 || (mix && reinterpret_cast<uintptr_t>(mix) % 16)) return hipErrorInvalidValue;
  if (!erase_args_ok(erase, C)) return hipErrorInvalidValue;
  const int np = (H / P) * (W / P);
  if (keep && (n_keep < 1 || n_keep > np)) return hipErrorInvalidValue;
  const int64_t total = (int64_t)B * (keep ? n_keep : np) * (Kp / 8);
  if (total <= 0) return hipSuccess;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  const auto kern = erase.rows ? (keep ? im2col_kernel<true, true, true> : im2col_kernel<true, false, true>)
                    : keep     ? (mix ? im2col_kernel<true, true> : im2col_kernel<false, true>)
                               : (mix ? im2col_kernel<true> : im2col_kernel<false>);
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, img, out, B, C, H, W, P, Kp, mix, keep, keep ? n_keep : 0, erase);
  return hipGetLastError();
}

extern "C" hipError_t pvr_im2col_u8(const uint8_t* img, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float* mean,
                                    const float* stdv, const float* geom, uint16_t* out, int B, int C, int Hs, int Ws, int H,
                                    int W, int P, int Kp, int vec, const pvr::MixRow* mix, const int* keep, int n_keep,
                                    pvr::EraseArgs erase, hipStream_t s) {
  using namespace pvr;
  if (mix && reinterpret_cast<uintptr_t>(mix) % 16) return hipErrorInvalidValue;
  if (!erase_args_ok(erase, C)) return hipErrorInvalidValue;
  if (Kp % 8 || P <= 0 || C < 1 || C > 4 || H % P || W % P || Kp < C * P * P || Hs < 1 || Ws < 1) return hipErrorInvalidValue;
  if (!geom && (Hs != H || Ws != W)) return hipErrorInvalidValue;
  if (vec && (geom || sx != 1 || P % 8 || reinterpret_cast<uintptr_t>(img) % 8 || sb % 8 || sc % 8 || sy % 8))
    return hipErrorInvalidValue;
  if (keep && (n_keep < 1 || n_keep > (H / P) * (W / P))) return hipErrorInvalidValue;
  const int64_t total = (int64_t)B * (keep ? n_keep : (H / P) * (W / P)) * (Kp / 8);
  if (total <= 0) return hipSuccess;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;  // 8 blocks per CU: a block's 256 x C table entries serve ~9 trips of its threads at b256
  U8Norm nrm;
  for (int c = 0; c < 4; ++c) {
    nrm.mean[c] = c < C ? mean[c] : 0.f;
    nrm.stdv[c] = c < C ? stdv[c] : 1.f;
  }
  const auto kern =
      erase.rows ? (keep ? (geom ? im2col_u8_kernel<true, true, true, true> : im2col_u8_kernel<false, true, true, true>)
                         : (geom ? im2col_u8_kernel<true, true, false, true> : im2col_u8_kernel<false, true, false, true>))
      : keep     ? (mix ? (geom ? im2col_u8_kernel<true, true, true> : im2col_u8_kernel<false, true, true>)
                        : (geom ? im2col_u8_kernel<true, false, true> : im2col_u8_kernel<false, false, true>))
                 : (mix ? (geom ? im2col_u8_kernel<true, true> : im2col_u8_kernel<false, true>)
                        : (geom ? im2col_u8_kernel<true, false> : im2col_u8_kernel<false, false>));
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, img, sb, sc, sy, sx, nrm, geom, out, B, C, Hs, Ws, H, W, P, Kp,
                     vec, mix, keep, keep ? n_keep : 0, erase);
  return hipGetLastError();
}

extern "C" hipError_t pvr_cls_rows(const float* cls, const float* pos, uint16_t* out, int B, int D, int64_t row_stride,
                                   pvr::DropSite drop, hipStream_t s) {
  using namespace pvr;
  if (B * D <= 0) return hipSuccess;
  int blocks = (B * D + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(cls_rows_kernel, dim3(blocks), dim3(256), 0, s, cls, pos, out, B, D, row_stride, drop.seed, drop.offset, drop.thr, drop.scale, (int64_t)0);
  return hipGetLastError();
}

extern "C" hipError_t pvr_patch_bwd(const uint16_t* dE, int B, int ntok, int D, float* ws, float* dpos, float* dcls,
                                    uint16_t* dconv, float* dbias, pvr::DropSite drop, const int* inv, int n_keep, hipStream_t s) {
  using namespace pvr;
  if (ntok * D <= 0 || B <= 0) return hipSuccess;
  if (D % 8) return hipErrorInvalidValue;
  if (inv && (n_keep < 1 || n_keep > ntok - 1)) return hipErrorInvalidValue;
  const int G = (B + PB_BAT - 1) / PB_BAT;  // ws holds G * ntok * D floats (host-checked)
  hipLaunchKernelGGL(inv ? patch_bwd_kernel<true> : patch_bwd_kernel<false>, dim3((ntok * (D / 8) + 255) / 256, G), dim3(256), 0, s, dE,
                     B, ntok, D, ws, dconv, drop.seed, drop.offset, drop.thr, drop.scale, inv, inv ? n_keep : 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // ws also holds the conv-bias partials of the reduction's token blocks, after the group sums
  const int RB = (ntok + PR_TOK - 1) / PR_TOK;
  float* part = dbias ? ws + (int64_t)G * ntok * D : nullptr;
  hipLaunchKernelGGL(patch_bwd_reduce_kernel, dim3((D / 8 + PR_CH - 1) / PR_CH, RB), dim3(256), 0, s,
                     ws, G, ntok, D, dpos, dcls, part);
  e = hipGetLastError();
  if (e != hipSuccess || !dbias) return e;
  hipLaunchKernelGGL(rows_reduce_kernel, dim3((D + 31) / 32), dim3(256), 0, s, part, RB, D, D, dbias, (float*)nullptr, (float*)nullptr);
  return hipGetLastError();
}

extern "C" int pvr_patch_bwd_groups(int B) { return (B + pvr::PB_BAT - 1) / pvr::PB_BAT; }

extern "C" hipError_t pvr_rows_reduce(const float* part, int R, int C, int seg, float* d0, float* d1, float* d2, hipStream_t s) {
  if (R <= 0 || C <= 0) return hipSuccess;
  if (seg <= 0 || C > 3 * seg) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pvr::rows_reduce_kernel, dim3((C + 31) / 32), dim3(256), 0, s, part, R, C, seg, d0, d1, d2);
  return hipGetLastError();
}

extern "C" int64_t pvr_patch_bwd_ws_floats(int B, int ntok, int D) {
  return ((int64_t)pvr_patch_bwd_groups(B) * ntok + (ntok + pvr::PR_TOK - 1) / pvr::PR_TOK) * D;
}

// Second half of the small-M split-K forward GEMM (few output tiles: serving-size batches): sum the
// S fp32 partial products ws[s][m][n] in a fixed order (deterministic) and apply the forward
// epilogue: + bias, exact-erf GELU (no derivative saved: inference), + residual, bf16 store.
// One thread per 4 consecutive columns of a row (N % 4 == 0).
namespace pvr {
namespace {
__global__ void __launch_bounds__(256) splitk_epilogue_kernel(const float* __restrict__ ws, int S, int64_t stride, int M, int N,
                                                              const float* __restrict__ bias, const uint16_t* __restrict__ resid,
                                                              int64_t ld_resid, int gelu, uint16_t* __restrict__ out, int64_t ldc) {
  const int n4 = N / 4;
  const int64_t total = (int64_t)M * n4;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int m = (int)(i / n4), n = (int)(i % n4) * 4;
    const float* src = ws + (int64_t)m * N + n;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    int s = 0;
    for (; s + 4 <= S; s += 4) {  // 4 independent loads in flight per trip
      const float4 b0 = *(const float4*)(src + (int64_t)s * stride);
      const float4 b1 = *(const float4*)(src + (int64_t)(s + 1) * stride);
      const float4 b2 = *(const float4*)(src + (int64_t)(s + 2) * stride);
      const float4 b3 = *(const float4*)(src + (int64_t)(s + 3) * stride);
      a.x += (b0.x + b1.x) + (b2.x + b3.x);
      a.y += (b0.y + b1.y) + (b2.y + b3.y);
      a.z += (b0.z + b1.z) + (b2.z + b3.z);
      a.w += (b0.w + b1.w) + (b2.w + b3.w);
    }
    for (; s < S; ++s) {
      const float4 b = *(const float4*)(src + (int64_t)s * stride);
      a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    float v[4] = {a.x, a.y, a.z, a.w};
    if (bias) {
      const float4 b = *(const float4*)(bias + n);
      v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
    if (gelu) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float g, gp;
        gelu_and_grad(v[r], g, gp);
        v[r] = g;
      }
    }
    if (resid) {
      const uint2 rr = *(const uint2*)(resid + (int64_t)m * ld_resid + n);
      v[0] += bf2f(rr.x & 0xFFFF); v[1] += bf2f(rr.x >> 16);
      v[2] += bf2f(rr.y & 0xFFFF); v[3] += bf2f(rr.y >> 16);
    }
    uint2 o; o.x = pack2bf(v[0], v[1]); o.y = pack2bf(v[2], v[3]);
    *(uint2*)(out + (int64_t)m * ldc + n) = o;
  }
}
}  // namespace
}  // namespace pvr

extern "C" hipError_t pvr_splitk_epilogue(const float* ws, int S, int64_t stride, int M, int N, const float* bias,
                                          const uint16_t* resid, int64_t ld_resid, int gelu, uint16_t* out, int64_t ldc,
                                          hipStream_t s) {
  using namespace pvr;
  if (M <= 0 || N <= 0) return hipSuccess;
  if (N % 4 || S < 1) return hipErrorInvalidValue;
  int64_t blocks = ((int64_t)M * (N / 4) + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ws, S, stride, M, N, bias, resid, ld_resid,
                     gelu, out, ldc);
  return hipGetLastError();
}
