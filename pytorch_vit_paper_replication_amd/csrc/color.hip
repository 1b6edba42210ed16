// Colour augmentation of a raw uint8 [B, 3, Hs, Ws] batch (3-Augment's grayscale / solarize / Gaussian
// blur, then brightness / contrast / saturation jitter; data/color_augment.py has the formulas). A pass
// of its own in front of the patchify kernels: it writes a new uint8 batch that im2col_u8 reads like
// the loader's. Three kernels, all through element strides (contiguous NCHW and channels_last alike):
//   * color_blur_kernel: the separable 13-tap blur of the op-3 samples, one LDS tile per workgroup;
//   * color_sum_kernel: the integer luma sum that the contrast step's mean needs;
//   * color_apply_kernel: the pointwise op and the three jitter steps, per pixel over its 3 channels.
// Every fp32 operation is rounded on its own, so the torch-op reference (color_reference) gives the same
// bytes. The contract(off) pragma alone does not do that here: the build's -ffp-contract=fast lets the
// backend fuse a multiply into the add behind it whatever the source says, and a fused product is not
// rounded (contrast 1.1 on a pixel 50 below the mean: 56 - 55.0000012 truncates to 0 where PIL has 1).
// mul_rn / mul2_rn below therefore pass every product that feeds an add through an empty asm.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace pvr {
namespace {

// a strided uint8 [B, 3, Hs, Ws] batch: element (b, c, y, x) at p[b * sb + c * sc + y * sy + x * sx]
struct U8View {
  uint8_t* p;
  int64_t sb, sc, sy, sx;
};

typedef float color_v2f __attribute__((ext_vector_type(2)));
// a * b as a value of its own (see the head of the file); the packed form keeps v_pk_mul_f32 / v_pk_add_f32
PVR_DEV float mul_rn(float a, float b) {
  float p = a * b;
  asm("" : "+v"(p));
  return p;
}
PVR_DEV color_v2f mul2_rn(float a, color_v2f b) {
  color_v2f p = b * a;
  asm("" : "+v"(p));
  return p;
}

PVR_DEV uint32_t color_luma(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16; }

// d + f * (v - d), clamped to [0, 255] and truncated: f = 1 gives v and f = 0 gives d exactly (d is an integer value)
PVR_DEV uint32_t color_blend(float d, uint32_t v, float f) {
#pragma clang fp contract(off)
  float t = (float)v - d;
  t = mul_rn(f, t);
  t = d + t;
  return (uint32_t)fminf(fmaxf(t, 0.f), 255.f);
}

// the pointwise ops (blur is color_blur_kernel's: its samples arrive here already blurred)
PVR_DEV void color_op(int op, uint32_t& r, uint32_t& g, uint32_t& b) {
  if (op == COLOR_GRAY) {
    r = g = b = color_luma(r, g, b);
  } else if (op == COLOR_SOLARIZE) {
    r = r < 128u ? r : 255u - r;
    g = g < 128u ? g : 255u - g;
    b = b < 128u ? b : 255u - b;
  }
}

// The jitter steps in the row's order, each on the bytes the step before it left. SUM: only the steps
// in front of contrast (what the luma sum is taken over); m: the contrast step's mean otherwise.
// Step codes 0 brightness, 1 contrast, 2 saturation, two bits each, first step lowest.
PVR_DEV uint32_t color_steps(int order) {
  // bcs, bsc, cbs, csb, sbc, scb
  constexpr uint64_t T = (0x24ull) | (0x18ull << 6) | (0x21ull << 12) | (0x09ull << 18) | (0x12ull << 24) | (0x06ull << 30);
  return (uint32_t)(T >> (6 * order)) & 0x3Fu;
}
template <bool SUM>
PVR_DEV void color_jitter(const ColorRow& row, uint32_t steps, float m, uint32_t& r, uint32_t& g, uint32_t& b) {
  for (int k = 0; k < 3; ++k) {
    const uint32_t st = (steps >> (2 * k)) & 3u;
    if (st == 0) {
      if (row.fb != 1.f) {
        r = color_blend(0.f, r, row.fb);
        g = color_blend(0.f, g, row.fb);
        b = color_blend(0.f, b, row.fb);
      }
    } else if (st == 1) {
      if constexpr (SUM) return;
      if (row.fc != 1.f) {
        r = color_blend(m, r, row.fc);
        g = color_blend(m, g, row.fc);
        b = color_blend(m, b, row.fc);
      }
    } else if (row.fs != 1.f) {
      const float l = (float)color_luma(r, g, b);
      r = color_blend(l, r, row.fs);
      g = color_blend(l, g, row.fs);
      b = color_blend(l, b, row.fs);
    }
  }
}

PVR_DEV uint32_t byte_of(const uint2& q, int j) { return ((j < 4 ? q.x : q.y) >> (8 * (j & 3))) & 0xFFu; }

// Blur tile: 32 x 64 outputs, a halo of COLOR_TAPS / 2 = 6 rows above and below, and the 80 bytes
// [x0 - 8, x0 + 72) of each row, so that the 8-byte chunks of the vector path stay aligned (the taps of
// output column lx are the LDS columns lx + 2 .. lx + 14).
constexpr int BLUR_H = 32, BLUR_W = 64, BLUR_R = COLOR_TAPS / 2, BLUR_ROWS = BLUR_H + 2 * BLUR_R, BLUR_COLS = 80;
static_assert(COLOR_TAPS == 13 && BLUR_W + 2 * 8 == BLUR_COLS, "the tile layout below is written for 13 taps");

// One workgroup per (sample, channel, tile); samples whose op is not blur leave at once (block-uniform).
// Source bytes (replicate-clamped) -> LDS; horizontal pass -> fp32 LDS tile; vertical pass -> output
// bytes in LDS -> the output batch. Each pass is t = t + w[i] * p over i = 0 .. 12 in that order.
__global__ void __launch_bounds__(256) color_blur_kernel(U8View in, U8View out, const ColorRow* __restrict__ rows, int Hs, int Ws,
                                                          int tx, int ty, int vec) {
#pragma clang fp contract(off)
  const int tiles = tx * ty;
  const int tile = blockIdx.x % tiles, bc = blockIdx.x / tiles, c = bc % 3, b = bc / 3;
  if (rows[b].op != COLOR_BLUR) return;
  __shared__ __attribute__((aligned(16))) uint8_t sbuf[BLUR_ROWS][BLUR_COLS];
  __shared__ __attribute__((aligned(16))) float tbuf[BLUR_ROWS][BLUR_W];
  __shared__ __attribute__((aligned(16))) uint8_t obuf[BLUR_H][BLUR_W];
  float w[COLOR_TAPS];
#pragma unroll
  for (int i = 0; i < COLOR_TAPS; ++i) w[i] = rows[b].w[i];
  const int tid = threadIdx.x;
  const int x0 = (tile % tx) * BLUR_W, y0 = (tile / tx) * BLUR_H;
  const uint8_t* src = in.p + b * in.sb + c * in.sc;
  if (vec) {  // sx == 1, Ws % 8 == 0, every row 8-byte aligned: a chunk lies wholly inside or wholly outside the row
    for (int it = tid; it < BLUR_ROWS * (BLUR_COLS / 8); it += 256) {
      const int r = it / (BLUR_COLS / 8), ch = it % (BLUR_COLS / 8);
      const int y = min(max(y0 - BLUR_R + r, 0), Hs - 1), gx = x0 - 8 + 8 * ch;
      const uint8_t* line = src + (int64_t)y * in.sy;
      uint2 q;
      if (gx >= 0 && gx < Ws) {
        q = *(const uint2*)(line + gx);
      } else {
        q.x = q.y = (uint32_t)line[gx < 0 ? 0 : Ws - 1] * 0x01010101u;
      }
      *(uint2*)&sbuf[r][8 * ch] = q;
    }
  } else {
    for (int it = tid; it < BLUR_ROWS * BLUR_COLS; it += 256) {
      const int r = it / BLUR_COLS, col = it % BLUR_COLS;
      const int y = min(max(y0 - BLUR_R + r, 0), Hs - 1), x = min(max(x0 - 8 + col, 0), Ws - 1);
      sbuf[r][col] = src[(int64_t)y * in.sy + (int64_t)x * in.sx];
    }
  }
  __syncthreads();
  // horizontal: 4 neighbouring outputs of one row from the 20 bytes at their aligned column
  for (int it = tid; it < BLUR_ROWS * (BLUR_W / 4); it += 256) {
    const int r = it / (BLUR_W / 4), xq = it % (BLUR_W / 4);
    const uint32_t* q = (const uint32_t*)&sbuf[r][4 * xq];
    float p[20];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const uint32_t d = q[k];
      p[4 * k] = (float)(d & 0xFFu);
      p[4 * k + 1] = (float)((d >> 8) & 0xFFu);
      p[4 * k + 2] = (float)((d >> 16) & 0xFFu);
      p[4 * k + 3] = (float)(d >> 24);
    }
    color_v2f a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
#pragma unroll
    for (int i = 0; i < COLOR_TAPS; ++i) {
      a01 = a01 + mul2_rn(w[i], (color_v2f){p[i + 2], p[i + 3]});
      a23 = a23 + mul2_rn(w[i], (color_v2f){p[i + 4], p[i + 5]});
    }
    *(float4*)&tbuf[r][4 * xq] = make_float4(a01.x, a01.y, a23.x, a23.y);
  }
  __syncthreads();
  // vertical: a lane owns one column and 8 rows (20 tile rows)
  {
    const int lx = tid & 63, ly0 = (tid >> 6) * 8;
    float t[8 + COLOR_TAPS - 1];
#pragma unroll
    for (int k = 0; k < 8 + COLOR_TAPS - 1; ++k) t[k] = tbuf[ly0 + k][lx];
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
      color_v2f o = {0.f, 0.f};
#pragma unroll
      for (int i = 0; i < COLOR_TAPS; ++i) o = o + mul2_rn(w[i], (color_v2f){t[k + i], t[k + 1 + i]});
      obuf[ly0 + k][lx] = (uint8_t)fminf(fmaxf(floorf(o.x + 0.5f), 0.f), 255.f);
      obuf[ly0 + k + 1][lx] = (uint8_t)fminf(fmaxf(floorf(o.y + 0.5f), 0.f), 255.f);
    }
  }
  __syncthreads();
  uint8_t* dst = out.p + b * out.sb + c * out.sc;
  if (vec) {
    const int ly = tid >> 3, ch = tid & 7;
    const int gy = y0 + ly, gx = x0 + 8 * ch;
    if (gy < Hs && gx < Ws) *(uint2*)(dst + (int64_t)gy * out.sy + gx) = *(const uint2*)&obuf[ly][8 * ch];
  } else {
    for (int it = tid; it < BLUR_H * BLUR_W; it += 256) {
      const int ly = it / BLUR_W, lx = it % BLUR_W;
      const int gy = y0 + ly, gx = x0 + lx;
      if (gy < Hs && gx < Ws) dst[(int64_t)gy * out.sy + (int64_t)gx * out.sx] = obuf[ly][lx];
    }
  }
}

// A workgroup covers COLOR_BLOCK_PX = 2048 pixels of one sample: 8 neighbouring pixels of one row per thread
// on the vector path (one 8-byte access per channel plane), 8 pixels 256 apart per thread otherwise.
// SUM: sums[b] += the luma of every pixel as the contrast step will see it (after the op and the jitter
// steps in front of contrast); samples whose contrast factor is 1 leave at once. Otherwise: the op and
// the whole jitter, stored to `out`. Blur samples read their blurred bytes from `out`.
template <bool SUM>
PVR_DEV void color_point(const U8View& in, const U8View& out, const ColorRow* __restrict__ rows, uint32_t* __restrict__ sums, int Hs,
                         int Ws, int bpi, int vec) {
#pragma clang fp contract(off)
  const int b = blockIdx.x / bpi, blk = blockIdx.x % bpi;
  const ColorRow row = rows[b];
  if constexpr (SUM) {
    if (row.fc == 1.f) return;
  }
  const int n = Hs * Ws, tid = threadIdx.x;
  const bool blurred = row.op == COLOR_BLUR;
  struct { int64_t sc, sy, sx; } sv = {blurred ? out.sc : in.sc, blurred ? out.sy : in.sy, blurred ? out.sx : in.sx};
  const uint8_t* src = blurred ? out.p + b * out.sb : in.p + b * in.sb;
  uint8_t* dst = out.p + b * out.sb;
  const uint32_t steps = color_steps(row.order);
  float m = 0.f;
  if constexpr (!SUM) {
    if (row.fc != 1.f) m = (float)(uint32_t)((2ull * sums[b] + (uint64_t)n) / (2ull * (uint64_t)n));
  }
  uint32_t acc = 0;
  if (vec) {
    const int p0 = (blk * 256 + tid) * 8;
    if (p0 < n) {
      const int y = p0 / Ws, x = p0 % Ws;
      const int64_t so = (int64_t)y * sv.sy + x;
      const uint2 qr = *(const uint2*)(src + so), qg = *(const uint2*)(src + sv.sc + so), qb = *(const uint2*)(src + 2 * sv.sc + so);
      uint2 orr = {0u, 0u}, og = orr, ob = orr;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint32_t r = byte_of(qr, j), g = byte_of(qg, j), bl = byte_of(qb, j);
        color_op(row.op, r, g, bl);
        color_jitter<SUM>(row, steps, m, r, g, bl);
        if constexpr (SUM) {
          acc += color_luma(r, g, bl);
        } else {
          const int sh = 8 * (j & 3);
          (j < 4 ? orr.x : orr.y) |= r << sh;
          (j < 4 ? og.x : og.y) |= g << sh;
          (j < 4 ? ob.x : ob.y) |= bl << sh;
        }
      }
      if constexpr (!SUM) {
        const int64_t d = (int64_t)y * out.sy + x;
        *(uint2*)(dst + d) = orr;
        *(uint2*)(dst + out.sc + d) = og;
        *(uint2*)(dst + 2 * out.sc + d) = ob;
      }
    }
  } else {
    for (int j = 0; j < 8; ++j) {
      const int p = blk * COLOR_BLOCK_PX + j * 256 + tid;
      if (p >= n) break;
      const int y = p / Ws, x = p % Ws;
      const int64_t so = (int64_t)y * sv.sy + (int64_t)x * sv.sx;
      uint32_t r = src[so], g = src[sv.sc + so], bl = src[2 * sv.sc + so];
      color_op(row.op, r, g, bl);
      color_jitter<SUM>(row, steps, m, r, g, bl);
      if constexpr (SUM) {
        acc += color_luma(r, g, bl);
      } else {
        const int64_t d = (int64_t)y * out.sy + (int64_t)x * out.sx;
        dst[d] = (uint8_t)r;
        dst[out.sc + d] = (uint8_t)g;
        dst[2 * out.sc + d] = (uint8_t)bl;
      }
    }
  }
  if constexpr (SUM) {
    // 2048 pixels of at most 255 each: far inside 32 bits. One atomic per workgroup.
    __shared__ uint32_t part[4];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) atomicAdd(&sums[b], part[0] + part[1] + part[2] + part[3]);
  }
}

__global__ void __launch_bounds__(256) color_sum_kernel(U8View in, U8View out, const ColorRow* __restrict__ rows,
                                                         uint32_t* __restrict__ sums, int Hs, int Ws, int bpi, int vec) {
  color_point<true>(in, out, rows, sums, Hs, Ws, bpi, vec);
}

__global__ void __launch_bounds__(256) color_apply_kernel(U8View in, U8View out, const ColorRow* __restrict__ rows,
                                                           uint32_t* __restrict__ sums, int Hs, int Ws, int bpi, int vec) {
  color_point<false>(in, out, rows, sums, Hs, Ws, bpi, vec);
}

}  // namespace
}  // namespace pvr

// blur (only with any_blur), then the cleared sums and the luma sum (only with any_sum), then apply
extern "C" hipError_t pvr_color_u8(const uint8_t* in, int64_t isb, int64_t isc, int64_t isy, int64_t isx, uint8_t* out, int64_t osb,
                                   int64_t osc, int64_t osy, int64_t osx, const pvr::ColorRow* rows, uint32_t* sums, int B, int Hs,
                                   int Ws, int vec, int any_blur, int any_sum, hipStream_t s) {
  using namespace pvr;
  if (B <= 0) return hipSuccess;
  const U8View vi = {const_cast<uint8_t*>(in), isb, isc, isy, isx}, vo = {out, osb, osc, osy, osx};
  const int64_t n = (int64_t)Hs * Ws;
  const int64_t bpi = (n + COLOR_BLOCK_PX - 1) / COLOR_BLOCK_PX;
  const int tx = (Ws + BLUR_W - 1) / BLUR_W, ty = (Hs + BLUR_H - 1) / BLUR_H;
  if (bpi * B >= (1ll << 31) || (int64_t)tx * ty * 3 * B >= (1ll << 31)) return hipErrorInvalidValue;
  if (any_blur) hipLaunchKernelGGL(color_blur_kernel, dim3((unsigned)(tx * ty * 3 * B)), dim3(256), 0, s, vi, vo, rows, Hs, Ws, tx, ty, vec);
  if (any_sum) {
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)B * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(color_sum_kernel, dim3((unsigned)(bpi * B)), dim3(256), 0, s, vi, vo, rows, sums, Hs, Ws, (int)bpi, vec);
  }
  hipLaunchKernelGGL(color_apply_kernel, dim3((unsigned)(bpi * B)), dim3(256), 0, s, vi, vo, rows, sums, Hs, Ws, (int)bpi, vec);
  return hipGetLastError();
}
