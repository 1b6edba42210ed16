// Patch embedding's input side: the im2col gather of an image batch into bf16 patch rows, from fp32
// images (im2col_kernel) or from uint8 images with the input pipeline's per-image work fused in
// (im2col_u8_kernel), and what three augmentations add to both while the pixels are gathered:
//   * MIX: mixup / CutMix;  * KEEP: patch dropout's subset of patches;  * ERASE: random erasing
// (one body for all pixel sources: mix_gather8 below), and the erase fill's noise as a kernel of its own.
#include "common.h"
#include "kernels.h"

namespace pvr {
namespace {

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

// What an ERASE kernel fills with, the same for all its threads: the erase argument, the site seed
// (*er.seed + er.offset in ERASE_PIXEL mode) and the [.][C][H][W] model image the fill's elements index
struct EraseSite {
  const EraseArgs& er;
  uint64_t sd;
  int C, H, W;
};

template <bool ERASE>
PVR_DEV uint64_t erase_seed(const EraseArgs& er) {
  if constexpr (ERASE) {
    if (er.mode == ERASE_PIXEL) return *er.seed + er.offset;
  }
  return 0;
}

// The fill of pixel (s, c, y, x) of the model image
PVR_DEV float erase_fill(const EraseSite& es, int s, int c, int y, int x) {
  if (es.er.mode == ERASE_PIXEL) return erase_normal(es.sd, (((uint64_t)s * es.C + c) * es.H + y) * es.W + x);
  return pick4(es.er.value, c);
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

// ---- The MIX / KEEP / ERASE gather, shared by both patchify kernels and all their pixel sources.
// A thread produces 8 consecutive k of one patch row, k = (c*P + ph)*P + pw, as fp32 before the bf16 cast.
// MIX: sample b's pixels are blended with / replaced by those of sample mix[b].partner while they
// are gathered (mixup / CutMix, see MixRow in kernels.h). A pixel whose weight is 0 or 1 is read from
// one sample only, so CutMix moves the bytes of the plain gather; mixup reads the input twice. From uint8
// the blend runs on the normalised fp32 values, each sample under its own crop box, so the no-GEOM table
// then holds fp32 values instead of their bf16 roundings.
// KEEP (patch dropout): only n_keep patches per sample are gathered. Output row r belongs to sample
// r / n_keep and holds patch keep[r] of it (keep [B][n_keep] int32, ascending per sample:
// patch_keep_kernel); the pixels, the padding and the mix plan (a box is in image pixels) are those of
// that patch in the plain kernel. It changes only which patch a row is, not the body below.
// ERASE (random erasing; only with MIX, whose plan may then be null = identity): a sample's own value
// inside its erase box er.rows[sample] is the fill (erase_fill) instead of the (from uint8: normalised)
// pixel, before the mix formula: the own and the partner pixel each test their own sample's box. An erased
// pixel is not loaded (eight erased pixels of the vector path load nothing); the loads that remain are
// those of the MIX kernel, inside the image. C <= 4 (the fill's per-channel value; host-checked).
// Every helper is PVR_DEV (force-inlined), so the fills of a thread's 8 pixels stay unrolled (16 call
// sites per code shape, 8 - 12 k instructions per instantiation): one rolled loop over the erased pixels
// is a third of the code but measured 10 % slower, a thread's fills then running one after the other
// (profiles/random_erasing/).

// The two samples one output row reads: side 0 = its own sample, side 1 = the partner
struct MixPair {
  int s[2];
  MixRow r;
  float oml;        // 1 - lam
  EraseRow box[2];  // ERASE: each side's erase box (else empty)
};

template <bool ERASE>
PVR_DEV MixPair mix_pair(const MixRow* __restrict__ mix, const EraseArgs& er, int b, int B) {
#pragma clang fp contract(off)
  MixPair m;
  m.r = ERASE ? erase_mix_row(mix, b, B) : mix_row(mix, b, B);
  m.s[0] = b; m.s[1] = m.r.partner;
  m.oml = 1.0f - m.r.lam;
  m.box[0] = m.box[1] = EraseRow{0, 0, 0, 0};
  if constexpr (ERASE) {
    m.box[0] = erase_row(er.rows, b);
    m.box[1] = erase_row(er.rows, m.r.partner);
  }
  return m;
}

// A pixel source answers "the fp32 value of a side's sample at model-image pixel (c, y, x)" in two steps:
// at(c, y, x) is what both sides share of that pixel (computed once, outside the branches that read),
// get(side, at) the value. With kRun8 it also reads the 8 pixels (c, y, x .. x + 7) as one vector access:
// at8 locates them, load8 fetches the raw bytes, lane(q, c, j) is pixel j of them, zero() a run not loaded.

// fp32 image [.][C][H][W]; base[side] = the side's sample
struct F32Source {
  static constexpr bool kRun8 = true;
  const float* base[2];
  int H, W;
  using At = int64_t;
  struct Vec {
    float4 lo, hi;
  };
  PVR_DEV At at(int c, int y, int x) const { return ((int64_t)c * H + y) * W + x; }
  PVR_DEV At at8(int c, int y, int x) const { return at(c, y, x); }
  PVR_DEV float get(int side, At off) const { return base[side][off]; }
  PVR_DEV static Vec zero() { return Vec{{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}; }
  PVR_DEV Vec load8(int side, At off) const {
    const float* src = base[side] + off;
    return Vec{*(const float4*)src, *(const float4*)(src + 4)};
  }
  PVR_DEV float lane(const Vec& q, int, int j) const {
    const float a[8] = {q.lo.x, q.lo.y, q.lo.z, q.lo.w, q.hi.x, q.hi.y, q.hi.z, q.hi.w};
    return a[j];
  }
};

// uint8 image by element strides, H x W = the source size, through the block's fp32 table lutf[c][byte]
struct U8TableSource {
  static constexpr bool kRun8 = true;
  const uint8_t* base[2];
  int64_t sc, sy, sx;
  const float (*lutf)[256];
  struct At {
    int c;
    int64_t off;
  };
  using Vec = uint2;
  PVR_DEV At at(int c, int y, int x) const { return At{c, c * sc + (int64_t)y * sy + (int64_t)x * sx}; }
  PVR_DEV At at8(int c, int y, int x) const { return At{c, c * sc + (int64_t)y * sy + x}; }  // a run has sx == 1
  PVR_DEV float get(int side, const At& a) const { return lutf[a.c][base[side][a.off]]; }
  PVR_DEV static Vec zero() { return Vec{0u, 0u}; }
  PVR_DEV Vec load8(int side, const At& a) const { return *(const uint2*)(base[side] + a.off); }
  PVR_DEV float lane(const Vec& q, int c, int j) const { return lutf[c][((j < 4 ? q.x : q.y) >> (8 * (j & 3))) & 0xFFu]; }
};

// uint8 image by element strides, resampled bilinearly: each side under its own sample's crop box
struct U8BilinearSource {
  static constexpr bool kRun8 = false;
  const uint8_t* base[2];
  int64_t sc, sy, sx;
  float4 g[2];
  float stepx[2], stepy[2];
  int Ws, Hs;
  const U8Norm& nrm;
  struct At {
    int c, y, x;
    float mean, stdv;
  };
  PVR_DEV At at(int c, int y, int x) const { return At{c, y, x, pick4(nrm.mean, c), pick4(nrm.stdv, c)}; }
  PVR_DEV float get(int side, const At& a) const {
    return u8_sample(base[side] + a.c * sc, sy, sx, g[side], stepx[side], stepy[side], a.x, a.y, Ws, Hs, a.mean, a.stdv);
  }
};

// The per-pixel rule: the own value unless inside the mix box, the partner's if inside or lam != 1
// (a side with weight 0 is not read), each replaced by the fill inside its own sample's erase box
// (an erased pixel is not read), then mix_value
template <bool ERASE, class Src>
PVR_DEV float mix_pixel(const Src& src, const MixPair& m, const EraseSite& es, int c, int y, int x) {
#pragma clang fp contract(off)
  const bool in = y >= m.r.by0 && y < m.r.by1 && x >= m.r.bx0 && x < m.r.bx1;
  const typename Src::At at = src.at(c, y, x);
  float a = 0.f, p = 0.f;
  if (!in) a = ERASE && erase_hit(m.box[0], x, y) ? erase_fill(es, m.s[0], c, y, x) : src.get(0, at);
  if (in || m.r.lam != 1.f) p = ERASE && erase_hit(m.box[1], x, y) ? erase_fill(es, m.s[1], c, y, x) : src.get(1, at);
  return mix_value(a, p, in, m.r.lam, m.oml);
}

// The rule over the 8 pixels (c, y, x .. x + 7) of one image row, each side read with at most one vector access.
// v is __restrict__ here and in mix_gather8: a helper is optimised on its own before it is inlined, and
// without it every store to v[j] could have changed *m's floats (branches then replace the blend's selects).
template <bool ERASE, class Src>
PVR_DEV void mix_run8(const Src& src, const MixPair& m, const EraseSite& es, int c, int y, int x, float (&__restrict__ v)[8]) {
#pragma clang fp contract(off)
  const bool yin = y >= m.r.by0 && y < m.r.by1;
  // ea / eq: the own / the partner pixel is used and erased. Without ERASE both are compile-time false and
  // the load conditions fold to "not all 8 inside the mix box" (n_in < 8) and "one inside, or lam != 1"
  // (n_in > 0 || lam != 1).
  bool in[8], ea[8], eq[8], need_a = false, need_p = false;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    in[j] = yin && x + j >= m.r.bx0 && x + j < m.r.bx1;
    const bool use_p = in[j] || m.r.lam != 1.f;
    ea[j] = ERASE && !in[j] && erase_hit(m.box[0], x + j, y);
    eq[j] = ERASE && use_p && erase_hit(m.box[1], x + j, y);
    need_a |= !in[j] && !ea[j];
    need_p |= use_p && !eq[j];
  }
  const typename Src::At at = src.at8(c, y, x);
  typename Src::Vec qa = Src::zero(), qp = Src::zero();
  if (need_a) qa = src.load8(0, at);
  if (need_p) qp = src.load8(1, at);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float fa = ea[j] ? erase_fill(es, m.s[0], c, y, x + j) : src.lane(qa, c, j);
    const float fp = eq[j] ? erase_fill(es, m.s[1], c, y, x + j) : src.lane(qp, c, j);
    v[j] = mix_value(fa, fp, in[j], m.r.lam, m.oml);
  }
}

// v = the 8 values k0 .. k0 + 7 of the patch at (y0, x0): one run of an image row where the source has
// vector access (`vec`) and the 8 lie below kc = C*P*P, else pixel by pixel with the zero padding past kc
template <bool ERASE, class Src>
PVR_DEV void mix_gather8(const Src& src, const MixPair& m, const EraseSite& es, bool vec, int k0, int kc, int P, int y0, int x0,
                         float (&__restrict__ v)[8]) {
  if constexpr (Src::kRun8) {
    if (vec && k0 + 8 <= kc) {
      const int c = k0 / (P * P), rem = k0 % (P * P), ph = rem / P, pw = rem % P;
      mix_run8<ERASE>(src, m, es, c, y0 + ph, x0 + pw, v);
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    v[j] = 0.f;
    if (k < kc) {
      const int c = k / (P * P), rem = k % (P * P), ph = rem / P, pw = rem % P;
      v[j] = mix_pixel<ERASE>(src, m, es, c, y0 + ph, x0 + pw);
    }
  }
}

// img [B][C][H][W] fp32 -> patches [B*np][Kp] bf16, k = (c*P + ph)*P + pw, zero padded to Kp.
// One thread per 8 consecutive k of a patch row: with P % 8 == 0 they are 8 consecutive pixels of
// one image row (two float4 loads, one 16-B store); the zero padding past C*P*P and other patch
// sizes (P = 14) take the per-element path. MIX, KEEP, ERASE: see mix_gather8 above.
template <bool MIX, bool KEEP = false, bool ERASE = false>
__global__ void __launch_bounds__(256) im2col_kernel(const float* __restrict__ img, uint16_t* __restrict__ out,
                                                      int B, int C, int H, int W, int P, int Kp,
                                                      const MixRow* __restrict__ mix, const int* __restrict__ keep, int n_keep,
                                                      EraseArgs er) {
  static_assert(MIX || !ERASE, "ERASE exists only together with MIX");
  const EraseSite es{er, erase_seed<ERASE>(er), C, H, W};
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
      const MixPair m = mix_pair<ERASE>(mix, er, b, B);
      const F32Source src{{img + (int64_t)b * C * H * W, img + (int64_t)m.r.partner * C * H * W}, H, W};
      mix_gather8<ERASE>(src, m, es, vec, k0, kc, P, y0, x0, v);
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
// MIX, KEEP, ERASE: see mix_gather8 above.
template <bool GEOM, bool MIX, bool KEEP = false, bool ERASE = false>
__global__ void __launch_bounds__(256) im2col_u8_kernel(const uint8_t* __restrict__ img, int64_t sb, int64_t sc, int64_t sy,
                                                         int64_t sx, U8Norm nrm, const float* __restrict__ geom,
                                                         uint16_t* __restrict__ out, int B, int C, int Hs, int Ws, int H, int W,
                                                         int P, int Kp, int vec, const MixRow* __restrict__ mix,
                                                         const int* __restrict__ keep, int n_keep, EraseArgs er) {
#pragma clang fp contract(off)
  static_assert(MIX || !ERASE, "ERASE exists only together with MIX");
  const EraseSite es{er, erase_seed<ERASE>(er), C, H, W};
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
      const MixPair m = mix_pair<ERASE>(mix, er, b, B);
      const uint8_t* src_p = img + m.r.partner * sb;
      float v[8];
      if constexpr (!GEOM) {
        const U8TableSource src{{src_b, src_p}, sc, sy, sx, lutf};
        mix_gather8<ERASE>(src, m, es, vec, k0, kc, P, py, px, v);
      } else {
        const float4 g = *(const float4*)(geom + (int64_t)b * 4), gp = *(const float4*)(geom + (int64_t)m.r.partner * 4);
        const U8BilinearSource src{{src_b, src_p}, sc, sy, sx, {g, gp},
                                   {(g.z - g.x) / (float)W, (gp.z - gp.x) / (float)W},
                                   {(g.w - g.y) / (float)H, (gp.w - gp.y) / (float)H}, Ws, Hs, nrm};
        mix_gather8<ERASE>(src, m, es, false, k0, kc, P, py, px, v);
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

}  // namespace
}  // namespace pvr

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
  // [erase][keep][mix]: an erase kernel is a MIX kernel, with a plan or without one
  static constexpr decltype(&im2col_kernel<false>) kernels[2][2][2] = {
      {{im2col_kernel<false>, im2col_kernel<true>}, {im2col_kernel<false, true>, im2col_kernel<true, true>}},
      {{im2col_kernel<true, false, true>, im2col_kernel<true, false, true>},
       {im2col_kernel<true, true, true>, im2col_kernel<true, true, true>}}};
  const auto kern = kernels[erase.rows != nullptr][keep != nullptr][mix != nullptr];
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
  // [geom][erase][keep][mix], as in pvr_im2col
  static constexpr decltype(&im2col_u8_kernel<false, false>) kernels[2][2][2][2] = {
      {{{im2col_u8_kernel<false, false>, im2col_u8_kernel<false, true>},
        {im2col_u8_kernel<false, false, true>, im2col_u8_kernel<false, true, true>}},
       {{im2col_u8_kernel<false, true, false, true>, im2col_u8_kernel<false, true, false, true>},
        {im2col_u8_kernel<false, true, true, true>, im2col_u8_kernel<false, true, true, true>}}},
      {{{im2col_u8_kernel<true, false>, im2col_u8_kernel<true, true>},
        {im2col_u8_kernel<true, false, true>, im2col_u8_kernel<true, true, true>}},
       {{im2col_u8_kernel<true, true, false, true>, im2col_u8_kernel<true, true, false, true>},
        {im2col_u8_kernel<true, true, true, true>, im2col_u8_kernel<true, true, true, true>}}}};
  const auto kern = kernels[geom != nullptr][erase.rows != nullptr][keep != nullptr][mix != nullptr];
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, s, img, sb, sc, sy, sx, nrm, geom, out, B, C, Hs, Ws, H, W, P, Kp,
                     vec, mix, keep, keep ? n_keep : 0, erase);
  return hipGetLastError();
}
