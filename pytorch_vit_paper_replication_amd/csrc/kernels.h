// The host-kernel interface: every extern "C" launcher (pvr_*) that the csrc/*.hip files define and
// bindings.cpp calls, declared once. Both sides include this header (hipcc and the host compiler),
// so a definition that drifts from its declaration no longer compiles (C linkage has no overloads).
// Plain C++: the HIP runtime API types only, no device code.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime_api.h>

#include "gemm_params.h"

namespace pvr {

// One row of the optimizer's param-group table, float32 [G][10] (optim/adam.py _group_array; word
// 7 holds an int). The weights of the new gradient in the moments, 1 - beta, are columns of their own,
// rounded once from the host's double: 1.f - beta1 on the fp32 beta would carry beta's absolute
// rounding (2^-25) as a relative error of 2^-25 / (1 - beta), 1.3e-5 at beta2 = 0.999, into v, which
// bc2_sqrt (from the exact beta2) does not share.
struct AdamGroup {
  float lr, beta1, beta2, eps, weight_decay;
  float bc1, bc2_sqrt;  // 1 - beta1^t, sqrt(1 - beta2^t)
  int decoupled;
  float one_minus_beta1, one_minus_beta2;
};
constexpr int ADAM_GROUP_COLS = 10;
static_assert(sizeof(AdamGroup) == ADAM_GROUP_COLS * sizeof(float), "AdamGroup is one float32 [10] row of the group table");

// Model EMA updated inside the Adam pass: buf (fp32, the layout of p) becomes
// decay * buf + one_minus_decay * p_new for every element the pass updates. pair: device
// {decay, one_minus_decay} (graph-captured steps, whose kernel arguments are frozen), or null: the
// by-value pair. buf null: no EMA.
struct AdamEma {
  float* buf = nullptr; const float* pair = nullptr; float decay = 0.f, one_minus_decay = 1.f;
};

// LAMB (lamb.hip) reads the same table. Its rows keep `decoupled` bit 0 clear and carry the group's
// always_adapt option in bit 1: a group takes the trust ratio ||w|| / ||u|| when its weight_decay is
// non-zero or this bit is set, and plain Adam steps otherwise. The Adam kernels never see such a row.
constexpr int LAMB_ALWAYS_ADAPT = 2;
// Elements of one chunk of the LAMB norm pass: one workgroup, 4 float4 per thread
constexpr int LAMB_CHUNK = 4096;

// SGD (sgd.hip) reads the same table too: lr, beta1 as the momentum, weight_decay, and in word 7 this bit
// for Nesterov momentum; every other column is ignored. A row with beta1 == 0 has no momentum buffer.
constexpr int SGD_NESTEROV = 4;

// A dropout site: the element's 16-bit hash of (*seed + offset) is kept iff >= thr = round(p * 65536);
// kept values scale by 65536 / (65536 - thr). seed null: no dropout.
struct DropSite {
  const uint64_t* seed = nullptr; uint64_t offset = 0; uint32_t thr = 0; float scale = 1.f;
};

// A drop-path (stochastic depth) site is a DropSite too, drawn per sample instead of per element:
// sample b is kept iff its 16-bit hash of (*seed + offset), index b, is >= thr, and a kept sample's
// residual branch scales by `scale`: s[b] = 0 or scale. A kernel takes it with dp_rows, the rows per
// sample (row r belongs to sample r / dp_rows). Sites: DROP_PATH_SITE + 2 i (attention branch of
// block i) and + 2 i + 1 (MLP branch), ops/fused_vit.py.

// Optional fp8 copy of a kernel's output (producer-side quantization of the delayed-scaling recipe):
// out[r][c] = fp8(v * (*scale)) (fmt 0 e4m3, 1 e5m2; row stride ld bytes), *amax = max(*amax, max|v|)
// (float bits). out null: none.
struct Fp8Copy {
  uint8_t* out = nullptr; int64_t ld = 0; const float* scale = nullptr; unsigned* amax = nullptr; int fmt = 0;
};

// One sample's row of a batch-mix plan (mixup / CutMix in the patchify kernels), int32 [B][8] on the
// device with lam's float bits in word 1 (data/batch_mix.py MixPlan); rows are 32 bytes, the base
// 16-byte aligned. With pre(s, ...) the fp32 value a kernel produces for sample s before its bf16
// cast, output pixel (b, c, y, x) becomes
//   pre(partner, c, y, x)                                   inside the half-open box, bx0 <= x < bx1 and by0 <= y < by1
//   pre(b, c, y, x)                                         else if lam == 1 (a select)
//   lam * pre(b, ...) + (1.0f - lam) * pre(partner, ...)    otherwise (fp32, each operation rounded on its own)
// Mixup: lam < 1, empty box. CutMix: lam == 1 and a box. Box coordinates are output (model image) pixels.
struct MixRow {
  int partner;  // in [0, B)
  float lam;
  int bx0, by0, bx1, by1;  // inside [0, W] x [0, H]
  int pad[2];  // not read by the kernels (MixPlan keeps the label weight's float bits in pad[0])
};
static_assert(sizeof(MixRow) == 32, "MixRow is one int32 [8] row of the plan tensor");

// One sample's row of a random-erasing plan, int32 [B][4] on the device (data/random_erasing.py
// ErasePlan), the base 16-byte aligned: the half-open box (x0, y0, x1, y1) in output (model image)
// pixels inside which the sample's own pre(s, c, y, x) is replaced by a fill before the mix formula
// above runs, so a partner's pixels are those of the partner's erased image. x0 == x1 or y0 == y1: the
// sample is not erased.
struct EraseRow {
  int x0, y0, x1, y1;  // inside [0, W] x [0, H], x0 <= x1, y0 <= y1 (host-validated: bindings.cpp erase_args)
};
static_assert(sizeof(EraseRow) == 16, "EraseRow is one int32 [4] row of the erase table");

// The fill: value[c] per channel (ERASE_CONST, the model's normalised space), or a standard normal
// per element from the counter hash (ERASE_PIXEL): erase_normal(*seed + offset, e) of patchify.hip
// with e = ((s * C + c) * H + y) * W + x, the element's index in the model image.
constexpr int ERASE_CONST = 0, ERASE_PIXEL = 1;
// The patchify kernels' erase argument. rows null: no erasing (the kernels that ran before it existed).
struct EraseArgs {
  const EraseRow* rows = nullptr; int mode = ERASE_CONST; float value[4] = {0.f, 0.f, 0.f, 0.f};
  const uint64_t* seed = nullptr; uint64_t offset = 0;  // ERASE_PIXEL: the step's counter and the site's offset
};

// One sample's row of a colour-augmentation plan, 20 words [B][20] on the device (data/color_augment.py
// ColorPlan, a float32 tensor whose first two words hold int32 bits), the base 16-byte aligned: the op, then
// the jitter steps brightness / contrast / saturation with factors fb / fc / fs in the order `order`
// (index into bcs, bsc, cbs, csb, sbc, scb). w: the blur's 13 normalised taps (COLOR_BLUR rows).
// Host-validated (bindings.cpp color_u8).
constexpr int COLOR_NONE = 0, COLOR_GRAY = 1, COLOR_SOLARIZE = 2, COLOR_BLUR = 3;
constexpr int COLOR_TAPS = 13;        // taps -6 .. 6: sigma <= COLOR_SIGMA_MAX keeps ceil(3 sigma) inside
constexpr float COLOR_SIGMA_MAX = 2.0f;
constexpr int COLOR_BLOCK_PX = 2048;  // pixels of one sample per workgroup of the sum and apply kernels
struct ColorRow {
  int op, order;
  float fb, fc, fs, sigma;
  float w[COLOR_TAPS];
  float pad;
};
static_assert(sizeof(ColorRow) == 80, "ColorRow is one 20-word row of the plan tensor");

// pvr_layernorm_bwd: dx = dres + LN'(dy); dw / db / dsum (each optional) accumulate dgamma, dbeta
// and the column sums of dx.
struct LnBwdParams {
  const uint16_t* dy; int64_t dy_stride;
  const uint16_t* x; int64_t x_stride;
  const float* mean; const float* rstd; const float* w;
  const uint16_t* dres; int64_t dres_stride;  // optional
  // dres_every > 1: only rows r % dres_every == 0 have a residual gradient, row r / dres_every of the
  // compact dres [ceil(rows / dres_every)][D] (the class-token rows); not with the fp8 copy q
  int dres_every;
  uint16_t* dx; int64_t dx_stride;
  float* dw; float* db; float* dsum;
  // dz (optional, needs drop.seed or dpath.seed): dz = s[row / dp_rows] * mask * scale * dx, the
  // dropout and / or drop-path backward of the branch that produced x's residual stream (either
  // factor alone is legal); dsum then receives dz's column sums. dz_nostore: only dz's fp8 copy is
  // written (needs q.out).
  uint16_t* dz; int64_t dz_stride; DropSite drop; int dz_nostore;
  // drop path of that branch (a per-sample DropSite, see above; seed null: none; not with the fp8 copy q)
  DropSite dpath; int dp_rows;
  Fp8Copy q;  // copy of the last-written gradient (dz if given, else dx); row stride and base % 8
  int rows, D;
  float* part;  // deterministic mode: [pvr_layernorm_bwd_blocks][3][D] partial rows (null: atomics)
};

// pvr_attn_bwd. dq_acc: f32 [B*N][D] zero-initialised workspace, required iff N > 256 (several key
// blocks per head); dq_rezero = 1 leaves it zeroed again afterwards (a persistent workspace reused
// across calls).
// dbias: optional f32 [B * nkb][3D] partial column sums of dQ | dK | dV (nkb = pvr_attn_bwd_key_blocks;
// every element is written), whose row sum is the in_proj bias gradient; on the pipelined path
// (pvr_attn_bwd_uses_pipe) the per-block partials described there.
// ws: f32 scratch of pvr_attn_bwd_ws_floats floats (the generic path's pre-pass outputs).
struct AttnBwdParams {
  const uint16_t* qkv; int64_t ld;
  const uint16_t* out; int64_t ld_o;
  const uint16_t* dout; int64_t ld_do;
  const float* lse;
  uint16_t* dqkv; int64_t ld_dq;
  float* dq_acc; int dq_rezero;
  float* dbias; float* bpart;  // bpart: see pvr_attn_bwd_part_rows
  float* ws;
  int B, N, H, D;
  float scale;
  DropSite drop;  // the forward's attention-probability dropout
  Fp8Copy q8;     // copy of dQKV (row stride and base % 4); q8_only: the bf16 dQKV is not stored
  int q8_only;
};

}  // namespace pvr

extern "C" {

// ---- gemm.hip, gemm_ws.hip
// Host entry. Returns hipSuccess, or hipErrorInvalidValue for an unsupported layout/epilogue pair.
hipError_t pvr_gemm(const pvr::GemmParams* p, hipStream_t s);
// The split-K tail plan a one-tile-per-workgroup GEMM of this shape gets (0: none): tests / tools.
int pvr_gemm_tail_split(int M, int N, int K, int elem_bytes, int max_units);
void pvr_set_fp8_persistent(int mode);
// Lean instantiations of the 256x256 ping-pong kernels (gemm_lean.h): 1 = a launch that matches the
// list takes its lean kernel (default), 0 = every launch takes the general kernel (A/B, tests).
void pvr_set_gemm_lean(int on);
// GemmLean bits of the kernel the most recent pvr_gemm launched (0: a general kernel)
int pvr_gemm_lean_last();
// 1 if the wave-specialized kernel takes this GEMM (k-contiguous bf16 operands, bf16-output
// epilogue without row remap / addend / fp8 copy, K a multiple of 64 and >= 256, 32-bit element
// indices, 31-bit buffer offsets)
int pvr_gemm_ws_ok(const pvr::GemmParams* p, int cus);
hipError_t pvr_gemm_ws(const pvr::GemmParams* p, int cus, hipStream_t s);
// 1 if tile config 15 (the wave-specialized kernel, gemm_ws.hip) runs this GEMM as given
int pvr_gemm_ws_takes(const pvr::GemmParams* p);

// ---- layernorm.hip
hipError_t pvr_layernorm_fwd(const uint16_t* x, int64_t x_stride, const float* w, const float* b, uint16_t* y, int64_t y_stride,
                             float* mean, float* rstd, int rows, int D, float eps, hipStream_t s);
void pvr_set_ln_fwd_q8_grid(int per_cu);
// pvr_layernorm_fwd plus the e4m3 copy q (row stride a multiple of 8) with the amax record (see
// ln_fwd_q8_kernel); y null: only the copy is written
hipError_t pvr_layernorm_fwd_q8(const uint16_t* x, int64_t x_stride, const float* w, const float* b, uint16_t* y, int64_t y_stride,
                                pvr::Fp8Copy q, float* mean, float* rstd, int rows, int D, float eps, hipStream_t s);
// grid of the LayerNorm backward (= the partial rows [blocks][3][D] of its deterministic mode)
int pvr_layernorm_bwd_blocks(int rows, int D);
hipError_t pvr_layernorm_bwd(const pvr::LnBwdParams* p, hipStream_t s);

// ---- elementwise.hip
hipError_t pvr_cast_f32_bf16(const float* in, uint16_t* out, int64_t n, hipStream_t s);
hipError_t pvr_splitk_reduce(const float* ws, int S, int64_t stride, float* out, int64_t n, int ocols, int wcols, int accumulate,
                             hipStream_t s);
hipError_t pvr_splitk_epilogue(const float* ws, int S, int64_t stride, int M, int N, const float* bias, const uint16_t* resid,
                               int64_t ld_resid, int gelu, uint16_t* out, int64_t ldc, hipStream_t s);
hipError_t pvr_pad_cols_bf16(const uint16_t* src, int rows, int cols, uint16_t* dst, int ld_dst, hipStream_t s);
// meta: int64 [nmat][5] = {src_off, dst_off, rows, cols, tile_prefix}; total_tiles = sum of tiles
hipError_t pvr_transpose_batched(const uint16_t* src, uint16_t* dst, const int64_t* meta, int nmat, int total_tiles, hipStream_t s);
// row groups of the column-sum kernel's grid (= the partial rows of its deterministic mode)
int pvr_colsum_part_rows(int rows);
// db (optional) += column sums of dy, or of dz = mask * scale * dy when drop.seed is set; dz
// (optional) receives that product, q its fp8 copy (row stride and base % 8); part: deterministic
// mode scratch [pvr_colsum_part_rows][N]; row_mul >= 1: row r takes the dropout mask of row r * row_mul
// (the compact class-token rows of a [rows * row_mul][N] tensor). dpath (seed null: none): the branch's
// drop-path site, dz = s[r / dp_rows] * mask * scale * dy (independent of row_mul: compact rows are
// samples, dp_rows = 1); not with the fp8 copy
hipError_t pvr_colsum(const uint16_t* dy, int64_t ld, int rows, int N, float* db, uint16_t* dz, int64_t ld_dz, pvr::DropSite drop,
                      pvr::Fp8Copy q, float* part, int row_mul, pvr::DropSite dpath, int dp_rows, hipStream_t s);
// s [B] f32 = the drop-path scale vector of a site (0 or dpath.scale per sample): diagnostics and the
// torch fallback's replay of the kernels' draws
hipError_t pvr_drop_path_scale(pvr::DropSite dpath, float* s_out, int B, hipStream_t s);
// d0/d1/d2[c % seg] += sum over the R rows of part[R][C] (row order: deterministic)
hipError_t pvr_rows_reduce(const float* part, int R, int C, int seg, float* d0, float* d1, float* d2, hipStream_t s);
// Patch dropout: keep [B][n_keep] (the kept patch indices of each sample, strictly ascending) and inv
// [B][np] (a patch's slot in its sample's keep row, -1: dropped) from the counter hash: sample b keeps the
// n_keep patches j with the smallest (rng_hash(*seed + offset, b * np + j), j) pairs. np <= 4096,
// 1 <= n_keep <= np, B * np < 2^32.
hipError_t pvr_patch_keep(const uint64_t* seed, uint64_t offset, int B, int np, int n_keep, int* keep, int* inv, hipStream_t s);
// out f32 [B][n_keep + 1][D]: row 1 + s of sample b = pos[keep[b][s] + 1], row 0 = pos[0] (pos [np + 1][D]; D % 4 == 0,
// 16-byte aligned bases): the embedding GEMM's position addend under patch dropout
hipError_t pvr_pos_gather(const float* pos, const int* keep, float* out, int B, int np, int n_keep, int D, hipStream_t s);
// The patchify kernels and the erase fill's noise (patchify.hip).
// mix (both patchify kernels; null: none): the batch's MixRow plan, host-validated (bindings.cpp mix_rows).
// keep (both; null: every patch): pvr_patch_keep's table; out then has B * n_keep rows, row r = patch
// keep[r] of sample r / n_keep
// erase (both; rows null: none): random erasing, the EraseRow table host-validated (bindings.cpp erase_args);
// the erase kernels are MIX kernels, in which a null mix is the identity plan
hipError_t pvr_im2col(const float* img, uint16_t* out, int B, int C, int H, int W, int P, int Kp, const pvr::MixRow* mix,
                      const int* keep, int n_keep, pvr::EraseArgs erase, hipStream_t s);
// strides in elements (= bytes); geom null: Hs == H and Ws == W. `vec`: the caller has checked the
// 8-byte load conditions on the base pointer and strides (bindings.cpp im2col_u8).
hipError_t pvr_im2col_u8(const uint8_t* img, int64_t sb, int64_t sc, int64_t sy, int64_t sx, const float* mean, const float* stdv,
                         const float* geom, uint16_t* out, int B, int C, int Hs, int Ws, int H, int W, int P, int Kp, int vec,
                         const pvr::MixRow* mix, const int* keep, int n_keep, pvr::EraseArgs erase, hipStream_t s);
// out f32 [n] = the ERASE_PIXEL fill of elements 0 .. n - 1 at site (*seed + offset): diagnostics and the
// tests' replay of the patchify kernels' noise (the same device function)
hipError_t pvr_erase_noise(const uint64_t* seed, uint64_t offset, float* out, int64_t n, hipStream_t s);
// Colour augmentation of a uint8 [B, 3, Hs, Ws] batch (csrc/color.hip): out = the op and the jitter of every
// sample's row, `in` untouched. Both batches through element strides; `vec`: the caller has checked the 8-byte
// access conditions on both (bindings.cpp color_u8). sums: uint32 [B] scratch, cleared on the stream here.
// any_blur / any_sum: some row has op COLOR_BLUR / a contrast factor other than 1 (else that kernel is not launched).
hipError_t pvr_color_u8(const uint8_t* in, int64_t isb, int64_t isc, int64_t isy, int64_t isx, uint8_t* out, int64_t osb, int64_t osc,
                        int64_t osy, int64_t osx, const pvr::ColorRow* rows, uint32_t* sums, int B, int Hs, int Ws, int vec,
                        int any_blur, int any_sum, hipStream_t s);
hipError_t pvr_cls_rows(const float* cls, const float* pos, uint16_t* out, int B, int D, int64_t row_stride, pvr::DropSite drop,
                        hipStream_t s);
// inv (null: none): pvr_patch_keep's slot table of a patch-dropout step. dE is then the compact
// [B][n_keep + 1][D] gradient (the dropout mask is that of the compact element index) and dconv
// [B * n_keep][D]; dpos / ws keep their ntok = np + 1 positions, exact zeros where no sample kept a patch
hipError_t pvr_patch_bwd(const uint16_t* dE, int B, int ntok, int D, float* ws, float* dpos, float* dcls, uint16_t* dconv,
                         float* dbias, pvr::DropSite drop, const int* inv, int n_keep, hipStream_t s);
int pvr_patch_bwd_groups(int B);
// floats of the scratch pvr_patch_bwd needs: the group sums and the conv-bias partials
int64_t pvr_patch_bwd_ws_floats(int B, int ntok, int D);

// ---- head.hip, xent.hip
hipError_t pvr_head_fwd(const uint16_t* tok, int64_t ld_tok, int B, int D, const float* gamma, const float* beta, float eps,
                        const float* W, const float* bias, int C, float* xhat, float* rstd, float* logits, hipStream_t s);
hipError_t pvr_head_bwd(const float* dl, const float* xhat, const float* rstd, const float* gamma, const float* beta, const float* W,
                        int B, int C, int D, int ntok, float* dW, float* db, float* dgamma, float* dbeta, float* dy, uint16_t* dtok,
                        float* part, hipStream_t s);
hipError_t pvr_scale_by(const float* x, const float* sc, float* y, int64_t n, hipStream_t s);
hipError_t pvr_mean(const float* x, int n, float* out, hipStream_t s);
hipError_t pvr_metrics_accum(float* sums, const float* loss, const int* correct, int B, hipStream_t s);
hipError_t pvr_rng_next(int64_t* rng, int64_t* seed, hipStream_t s);
hipError_t pvr_zero_f32(float* x, int64_t n, hipStream_t s);
hipError_t pvr_xent(const float* logits, int64_t ld, const int64_t* labels, int B, int C, float* loss_rows, float* dlogits,
                    int* correct, float grad_scale, hipStream_t s);
// Soft-target rows q = (1 - eps) * (lam * onehot(ya) + (1 - lam) * onehot(yb)) + eps / C (mixed labels,
// label smoothing): loss_rows = -sum_c q_c log softmax_c, dlogits = (softmax - q) * grad_scale,
// correct = (argmax == ya). lam = 1, eps = 0, yb = ya gives pvr_xent's bits. A row whose ya or yb is
// outside [0, C) has zero loss and gradient.
hipError_t pvr_xent_soft(const float* logits, int64_t ld, const int64_t* ya, const int64_t* yb, const float* lam, float eps, int B,
                         int C, float* loss_rows, float* dlogits, int* correct, float grad_scale, hipStream_t s);

// ---- bce.hip
// Binary cross-entropy with logits against pvr_xent_soft's target rows q, or against q > thr when
// thr >= 0 (thr < 0: off): loss_rows = row_scale * sum_c (log(1 + exp(x_c)) - x_c t_c), dlogits =
// (sigmoid(x) - t) * grad_scale, correct = (argmax == ya). Invalid rows as in pvr_xent_soft.
hipError_t pvr_bce(const float* logits, int64_t ld, const int64_t* ya, const int64_t* yb, const float* lam, float eps, float thr,
                   int B, int C, float row_scale, float* loss_rows, float* dlogits, int* correct, float grad_scale, hipStream_t s);

// ---- layerscale.hip
// LayerScale folded into the last Linear of a residual branch. One launch over every scaled weight: meta
// int64 [nmat][8] = {W offset, g offset, b offset (in master, fp32), R, C, offset in w16 / wt16, offset in
// bhat, tile prefix}; R, C and every offset multiples of 8; total_tiles = sum of 64x64 tiles. Writes
// w16 [R][C] = bf16_rne(fl32(g[i] * W[i][j])), wt16 [C][R] the same values transposed, bhat [R] = fl32(g[i] * b[i]).
hipError_t pvr_layerscale_fold(const float* master, uint16_t* w16, uint16_t* wt16, float* bhat, const int64_t* meta, int nmat,
                               int total_tiles, hipStream_t s);
// The gradients of (W [R][C], b [R], g [R]) from those of the folded pair, dWh [R][C] and dbh [R]:
// gW += g[i] * dWh, gb += g[i] * dbh, gg[i] += dot(dWh[i], W[i]) + dbh[i] * b[i]; a null destination is
// skipped. One workgroup per row, no atomics. vec: every pointer is 16-byte aligned and C % 4 == 0.
hipError_t pvr_layerscale_unfold(const float* dWh, const float* dbh, const float* W, const float* b, const float* g, float* gW,
                                 float* gb, float* gg, int R, int C, int vec, hipStream_t s);

// ---- optim.hip
int pvr_norm_partial_blocks();
// workspace: NORM_BLOCKS floats. out: 3 floats.
hipError_t pvr_grad_norm(const float* g, int64_t n, float max_norm, float* workspace, float* out, hipStream_t s);
// groups: device table, or null with host_groups [ngroups <= 8] copied into the kernel arguments
hipError_t pvr_adam(float* p, const float* g, float* m, float* v, uint16_t* shadow, int64_t n, const int64_t* seg_start,
                    const int* seg_group, int nseg, const pvr::AdamGroup* groups, const pvr::AdamGroup* host_groups, int ngroups,
                    const float* clip, int skip_nonfinite, pvr::AdamEma ema, hipStream_t s);
hipError_t pvr_scale_by_clip(float* g, int64_t n, const float* clip, hipStream_t s);
// Adam with the transposed bf16 shadow (adam_t_kernel): tmeta int64 [nmat][6], fmeta int64 [nflat][4]
// (see the kernel), flat4 = float4s covered by fmeta.
hipError_t pvr_adam_t(float* p, const float* g, float* m, float* v, uint16_t* shadow, uint16_t* shadow_t, const int64_t* tmeta,
                      int nmat, int ntiles, const int64_t* fmeta, int nflat, int64_t flat4, const pvr::AdamGroup* groups,
                      const pvr::AdamGroup* host_groups, int ngroups, const float* clip, int skip_nonfinite, pvr::AdamEma ema,
                      hipStream_t s);

// ---- lamb.hip
// LAMB on the flat buffers of pvr_adam, three launches. Segment i is one parameter tensor; seg_group
// int32 [nseg] its param group (-1 frozen). groups / host_groups / clip / skip_nonfinite as in pvr_adam;
// all three return at once on a skipped non-finite step.
// 1: moments. chunks int64 [nchunks][3] {flat start, elements (multiple of 4, <= LAMB_CHUNK), segment};
// a chunk lies inside one trainable segment. Writes m, v and partial f32 [nchunks][2] = the chunk's
// {sum p^2, sum u^2}, u = (m / bc1) / (sqrt(v) / bc2_sqrt + eps) + weight_decay * p. n: elements of the buffers.
hipError_t pvr_lamb_moments(const float* p, const float* g, float* m, float* v, int64_t n, const int64_t* chunks, int nchunks,
                            const int* seg_group, int nseg, float* partial, const pvr::AdamGroup* groups,
                            const pvr::AdamGroup* host_groups, int ngroups, const float* clip, int skip_nonfinite, hipStream_t s);
// 2: trust f32 [nseg][3] = {||w||, ||u||, r} per trainable segment from its chunks' partials, summed in
// double in a fixed order. seg_chunks int64 [nseg][2] {first chunk, chunks}; rows of frozen segments stay.
hipError_t pvr_lamb_ratio(const float* partial, int nchunks, const int64_t* seg_chunks, const int* seg_group, int nseg, float* trust,
                          const pvr::AdamGroup* groups, const pvr::AdamGroup* host_groups, int ngroups, const float* clip,
                          int skip_nonfinite, hipStream_t s);
// 3: p -= lr * trust[seg].r * u with u recomputed from the new m, v; bf16 shadow, W^T and the model EMA
// as pvr_adam / pvr_adam_t write them. ntiles > 0: the tile form, tmeta int64 [nmat][7] and fmeta int64
// [nflat][5] = pvr_adam_t's rows with the segment index appended. ntiles == 0: the segment-table form
// over n elements (seg_start int64 [nseg]; shadow optional).
hipError_t pvr_lamb_update(float* p, const float* m, const float* v, uint16_t* shadow, uint16_t* shadow_t, int64_t n,
                           const int64_t* seg_start, const int* seg_group, int nseg, const int64_t* tmeta, int nmat, int ntiles,
                           const int64_t* fmeta, int nflat, int64_t flat4, const float* trust, const pvr::AdamGroup* groups,
                           const pvr::AdamGroup* host_groups, int ngroups, const float* clip, int skip_nonfinite, pvr::AdamEma ema,
                           hipStream_t s);

// ---- sgd.hip
// SGD with momentum (torch.optim.SGD, dampening 0) on the flat buffers of pvr_adam, one launch: per element
// g' = g * clip[1] (+ weight_decay * p), buf = beta1 * buf + g' (rows with beta1 != 0 only: buf of a row with
// beta1 == 0 is neither read nor written), d = g' + beta1 * buf with SGD_NESTEROV, else buf (g' without
// momentum), p -= lr * d; bf16 shadow, W^T and the model EMA as pvr_adam / pvr_adam_t write them.
// pvr_sgd_blocks: the segment-table form's grid cap (its grid-stride loop covers blocks * 256 float4 per trip).
int pvr_sgd_blocks();
hipError_t pvr_sgd(float* p, const float* g, float* buf, uint16_t* shadow, int64_t n, const int64_t* seg_start, const int* seg_group,
                   int nseg, const pvr::AdamGroup* groups, const pvr::AdamGroup* host_groups, int ngroups, const float* clip,
                   int skip_nonfinite, pvr::AdamEma ema, hipStream_t s);
// The tile form: pvr_adam_t's tables (tmeta int64 [nmat][6], fmeta int64 [nflat][4]).
hipError_t pvr_sgd_t(float* p, const float* g, float* buf, uint16_t* shadow, uint16_t* shadow_t, const int64_t* tmeta, int nmat,
                     int ntiles, const int64_t* fmeta, int nflat, int64_t flat4, const pvr::AdamGroup* groups,
                     const pvr::AdamGroup* host_groups, int ngroups, const float* clip, int skip_nonfinite, pvr::AdamEma ema,
                     hipStream_t s);

// ---- fp8.hip
hipError_t pvr_fp8_quant(const uint16_t* x, int64_t ldx, uint8_t* y, int64_t ldy, int64_t rows, int cols, const float* qscale,
                         unsigned* amax, int fmt, hipStream_t s);
hipError_t pvr_fp8_quant_multi(const int64_t* segs, int nseg, int64_t nchunks, const float* qscale, unsigned* amax, int fmt,
                               int amax_only, hipStream_t s);
hipError_t pvr_fp8_quant_t(const uint16_t* x, int64_t ldx, uint8_t* y, int64_t ldy, int T, int C, const float* qscale, int fmt,
                           hipStream_t s);
hipError_t pvr_fp8_transpose(const uint8_t* x, int64_t ldx, uint8_t* y, int64_t ldy, int T, int C, hipStream_t s);
hipError_t pvr_fp8_dequant(const uint8_t* x, float* y, int64_t n, const float* dscale, int fmt, hipStream_t s);
hipError_t pvr_fp8_scale_update(float* hist, int H, unsigned* amax, float* qscale, float* dscale, const float* fmax, int s0, int s1,
                                float margin_mul, hipStream_t s);

// ---- attention.hip
void pvr_set_attn_fwd_qg(int qg);
void pvr_set_attn_fwd_head_qf(int qf);
void pvr_set_attn_prep_xcd(int on);
// diagnostic builds (-DPVR_ATTN_STAMPS): where the backward writes its phase stamps (null: nowhere)
void pvr_set_attn_dbg(void* p);
int pvr_attn_head_dim_supported(int dh);
// drop: attention-probability dropout (see AttnDrop); the backward must get the same site.
// q8: e4m3 copy of the output (row stride and base % 4); q8_only (inference): the bf16 out is unwritten
hipError_t pvr_attn_fwd(const uint16_t* qkv, int64_t ld, uint16_t* out, int64_t ld_o, float* lse, int B, int N, int H, int D,
                        float scale, pvr::DropSite drop, pvr::Fp8Copy q8, int q8_only, hipStream_t s);
// ws: f32 [S][H][2 * DH] scratch, S = pvr_attn_dbias_splits(B, NQ); part f32 [B*H][NQ][3 * DH]
int pvr_attn_dbias_splits(int B, int NQ);
hipError_t pvr_attn_dbias_reduce(const float* part, float* ws, float* dbias, int B, int H, int NQ, int D, hipStream_t s);
int pvr_attn_bwd_waves(int N);
int pvr_attn_bwd_key_blocks(int N);
// 1 if pvr_attn_bwd needs the zero-initialised f32 dQ workspace for this shape (det: deterministic
// mode, where such shapes sum per-key-block dQ slabs in a fixed order instead: no workspace)
int pvr_attn_bwd_needs_dq_acc(int N, int dh, int dbias, int drop, int det);
// floats of the f32 scratch pvr_attn_bwd needs (per-query delta and, on the lastkey path, ds_last;
// dQ slabs on the tail-split path, and in deterministic mode (det) on multi-key-block shapes without it)
int64_t pvr_attn_bwd_ws_floats(int B, int N, int H, int D, int dbias, int drop, int det);
// 1 if pvr_attn_bwd can write dQKV's e5m2 copy (q8.out) for this shape: the generic kernels must
// write every final dQ value
int pvr_attn_bwd_q8_ok(int N, int drop);
// 1 if pvr_attn_bwd takes the pipelined whole-head backward for this shape and these layouts; its
// dbias is then f32 [B*H][ceil(N/32)][192] partials instead: per (batch, head, 32-query block) the
// column sums of dQ over its two 16-query halves (2 x 64, the head's q-bias slice; summed) and of dO
// (64: the v-bias slice, sum_k dV = sum_q dO since softmax rows sum to 1); the k-bias gradient is
// exactly 0 (sum_k dS = 0 per query)
int pvr_attn_bwd_uses_pipe(int B, int N, int H, int D, int64_t ld, int64_t ld_do, int64_t ld_o, int64_t ld_dq, int drop);
// Rows R of the f32 [B*H][R][3*dh] bias-gradient partials (q half 0 | q half 1 | v) that pvr_attn_bwd
// writes for this shape: pipelined kernel (into `dbias`): R = 32-query blocks; generic kernel (into
// `bpart`): R = 1 where attn_bwd_bpart_ok; 0: none (`dbias` then means the generic kernel's
// [B * key blocks][3D] layout).
int pvr_attn_bwd_part_rows(int B, int N, int H, int D, int64_t ld, int64_t ld_do, int64_t ld_o, int64_t ld_dq, int drop);
hipError_t pvr_attn_bwd(const pvr::AttnBwdParams* p, hipStream_t s);
// Class-token attention (the last encoder block of a classifier: one query, token 0, per image and
// head; no attention dropout). 1 if the kernels take this shape (any N in [1, 8192], the head dims above)
int pvr_attn_cls_ok(int N, int dh);
// out [B][D] (row stride ld_o) = softmax(q_0 K^T * scale) V per (image, head), lse f32 [B*H]
hipError_t pvr_attn_cls_fwd(const uint16_t* qkv, int64_t ld, uint16_t* out, int64_t ld_o, float* lse, int B, int N, int H, int D,
                            float scale, hipStream_t s);
// dqkv [B*N][3D] (every element written: dQ rows other than token 0 are zero) from dout / o [B][D] and
// lse [B*H]; dq0 f32 [B][D] receives dQ_0 unrounded
hipError_t pvr_attn_cls_bwd(const uint16_t* qkv, int64_t ld, const uint16_t* o, int64_t ld_o, const uint16_t* dout, int64_t ld_do,
                            const float* lse, uint16_t* dqkv, int64_t ld_dq, float* dq0, int B, int N, int H, int D, float scale,
                            hipStream_t s);
// dbias [3D] += the in_proj bias gradient: column sums of dq0 (q slice) and of dout (v slice), images in order
hipError_t pvr_attn_cls_dbias(const float* dq0, const uint16_t* dout, int64_t ld_do, float* dbias, int B, int D, hipStream_t s);

}  // extern "C"
