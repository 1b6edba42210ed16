#include <cstdlib>
// pybind11 / ATen bindings for the gfx950 kernels. Every entry point launches on PyTorch's current
// HIP stream (so it composes with torch streams, events and hipGraph capture) and validates dtypes,
// shapes and strides before touching device memory.
#include <algorithm>
#include <map>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace {

hipStream_t stream() { return c10::hip::getCurrentHIPStream().stream(); }
// Per-(device, stream) scratch caches are keyed by the stream's id (a pooled raw handle can be
// reused by a different stream) and live in heap maps that free_scratch() empties (never in
// static-storage destructors, which would run after the HIP runtime's teardown).
using ScratchKey = std::pair<int, int64_t>;
ScratchKey scratch_key(int dev) { return std::make_pair(dev, (int64_t)c10::hip::getCurrentHIPStream().id()); }
template <class T>
std::map<ScratchKey, T>& scratch_map() {
  static auto* m = new std::map<ScratchKey, T>();
  return *m;
}
struct SkCounters { torch::Tensor t; };
struct DetWs { torch::Tensor t; };
struct DqWs { torch::Tensor t; };
struct AttnWs { torch::Tensor t; };

// compute units of the current device (the persistent kernels' grid)
int num_cus() {
  static std::map<int, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  auto it = cache.find(dev);
  if (it != cache.end()) return it->second;
  hipDeviceProp_t prop;
  int n = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  cache[dev] = n;
  return n;
}

void check(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "pvr kernel '", what, "' failed: ", hipGetErrorString(e));
}

const uint16_t* bf(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bfloat16, got ", t.scalar_type());
  return reinterpret_cast<const uint16_t*>(t.data_ptr());
}
uint16_t* bf_mut(torch::Tensor& t, const char* name) { return const_cast<uint16_t*>(bf(t, name)); }
const float* f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32, got ", t.scalar_type());
  return t.data_ptr<float>();
}
float* f32_mut(torch::Tensor& t, const char* name) { return const_cast<float*>(f32(t, name)); }

template <class T>
T* opt_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() && t->defined() ? reinterpret_cast<T*>(t->data_ptr()) : nullptr;
}

// 2-D row-major view check: last-dim contiguous, returns leading dimension (elements)
int64_t ld_of(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() == 2, name, " must be 2-D");
  TORCH_CHECK(t.stride(1) == 1, name, " must have unit stride in its last dim");
  TORCH_CHECK(t.stride(0) % 8 == 0 || t.size(0) == 1, name, " leading dimension must be a multiple of 8 elements");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
  return t.size(0) == 1 ? t.size(1) : t.stride(0);
}

// The dropout site of every kernel that draws or recomputes a mask (pvr::DropSite): the only place
// that derives thr and scale from drop_p. drop_p == 0: no dropout (seed unread).
pvr::DropSite drop_args(const c10::optional<torch::Tensor>& seed, int64_t seed_offset, double drop_p, const char* what) {
  pvr::DropSite d;
  d.offset = (uint64_t)seed_offset;
  if (drop_p > 0.0) {
    TORCH_CHECK(seed.has_value() && seed->defined() && seed->is_cuda() && seed->scalar_type() == torch::kInt64 && seed->numel() >= 1,
                what, ": dropout needs an int64 seed tensor on the GPU");
    d.seed = reinterpret_cast<const uint64_t*>(seed->data_ptr());
    d.thr = (uint32_t)llround(drop_p * 65536.0);
    if (d.thr > 65535) d.thr = 65535;
    d.scale = (float)(65536.0 / (65536.0 - d.thr));
  }
  return d;
}
// A drop-path site (per-sample DropSite, csrc/kernels.h): the same thr / scale rule as drop_args.
// dp_p == 0: none (seed unread).
pvr::DropSite drop_path_args(const c10::optional<torch::Tensor>& seed, int64_t seed_offset, double dp_p, int64_t dp_rows,
                             const char* what) {
  TORCH_CHECK(dp_p >= 0.0 && dp_p <= 1.0, what, ": drop_path rate must be in [0, 1]");
  if (dp_p > 0.0) TORCH_CHECK(dp_rows >= 1 && dp_rows < (int64_t(1) << 31), what, ": drop_path needs rows per sample >= 1");
  return drop_args(seed, seed_offset, dp_p, what);
}
// GemmParams keeps the site flat (the GEMM kernels take the struct by value); untouched without dropout
void set_drop(pvr::GemmParams& p, const pvr::DropSite& d) {
  if (!d.seed) return;
  p.seed_ptr = d.seed; p.seed_offset = d.offset; p.drop_thr = d.thr; p.drop_scale = d.scale;
}

// The optional fp8 copy of a kernel's [rows, cols] output (pvr::Fp8Copy; q_fmt 0 e4m3, 1 e5m2):
// q_out uint8 with its row stride and base pointer multiples of `align` bytes, q_scale the delayed
// scale (f32), q_amax the amax record (int32 holding float bits). q_out None: no copy.
pvr::Fp8Copy fp8_copy(const c10::optional<torch::Tensor>& q_out, const c10::optional<torch::Tensor>& q_scale,
                      const c10::optional<torch::Tensor>& q_amax, int64_t q_fmt, int64_t rows, int64_t cols, int64_t align,
                      const char* what) {
  pvr::Fp8Copy q;
  q.fmt = (int)q_fmt;
  if (!q_out.has_value() || !q_out->defined()) return q;
  TORCH_CHECK(q_out->is_cuda() && q_out->scalar_type() == torch::kUInt8 && q_out->dim() == 2 && q_out->stride(1) == 1 &&
                  q_out->size(0) >= rows && q_out->size(1) >= cols && q_out->stride(0) % align == 0 &&
                  reinterpret_cast<uintptr_t>(q_out->data_ptr()) % align == 0,
              what, ": q_out must be uint8 [>= ", rows, "][>= ", cols, "] with unit column stride, row stride and base multiples of ", align);
  TORCH_CHECK(q_scale.has_value() && q_scale->defined() && q_amax.has_value() && q_amax->defined() && q_amax->is_cuda() &&
                  q_amax->scalar_type() == torch::kInt32 && (q_fmt == 0 || q_fmt == 1),
              what, ": q_out needs q_scale (f32), q_amax (int32 on the GPU) and q_fmt 0 / 1");
  q.out = q_out->data_ptr<uint8_t>();
  q.ld = q_out->stride(0);
  q.scale = f32(*q_scale, "q_scale");
  q.amax = reinterpret_cast<unsigned*>(q_amax->data_ptr());
  return q;
}

// Split-K tail of the one-tile-per-workgroup GEMMs (GemmParams::tail_*): per (device, stream) a
// slab workspace of CUs x 256x256 fp32 partial tiles and CUs arrival counters (zeroed once; each
// launch leaves them zero). GEMMs on one stream are serialised, so they share the buffers.
bool g_gemm_tail = true;
struct TailBufs {
  torch::Tensor ws, cnt;
};
void attach_tail(pvr::GemmParams& p, const torch::Tensor& like) {
  if (!g_gemm_tail) return;
  auto& bufs = scratch_map<TailBufs>();
  const auto key = scratch_key((int)like.get_device());
  auto it = bufs.find(key);
  if (it == bufs.end()) {
    const int64_t cus = num_cus();
    TailBufs b;
    b.ws = torch::empty({cus * 65536}, like.options().dtype(torch::kFloat32));
    b.cnt = torch::zeros({cus}, like.options().dtype(torch::kInt32));
    it = bufs.emplace(key, b).first;
  }
  p.tail_ws = it->second.ws.data_ptr<float>();
  p.tail_cnt = reinterpret_cast<unsigned*>(it->second.cnt.data_ptr<int32_t>());
  p.tail_ws_elems = it->second.ws.numel();
  p.tail_cnt_elems = (int)it->second.cnt.numel();
}
void set_gemm_tail(bool on) { g_gemm_tail = on; }
// Lean GEMM instantiations (csrc/gemm_lean.h) on / off (_ext.py turns them off for PVR_GEMM_LEAN=0)
void set_gemm_lean(bool on) { pvr_set_gemm_lean(on ? 1 : 0); }

// Counters of the in-launch split-K reduction (GemmParams::sk_*): per (device, stream) two words
// per output tile plus a timeout count, zeroed once; every launch leaves the tile words zero.
constexpr int g_sk_tiles = 4096;
torch::Tensor& splitk_counters(const torch::Tensor& like) {
  auto& bufs = scratch_map<SkCounters>();
  const auto key = scratch_key((int)like.get_device());
  auto it = bufs.find(key);
  if (it == bufs.end()) it = bufs.emplace(key, SkCounters{torch::zeros({2 * g_sk_tiles + 4}, like.options().dtype(torch::kInt32))}).first;
  return it->second.t;
}
// spin timeouts of the in-launch split-K reduction on the current stream (0 unless a split's
// workgroups were not co-resident); reset = true zeroes the count
int64_t splitk_timeouts(torch::Tensor like, bool reset) {
  torch::Tensor& c = splitk_counters(like);
  const int64_t v = c[2 * g_sk_tiles].item<int32_t>();
  if (reset) c[2 * g_sk_tiles].zero_();
  return v;
}
// fewest K-tiles per split-tail part: 12 (6 / 4 / 3 measured no better or worse on the short-K
// GEMMs, profiles/r4/ab14/tail_kt.log)
constexpr int g_tail_min_kt = 12;

// Deterministic mode (set_deterministic): the reductions that otherwise add float atomics in
// arrival order (LayerNorm backward dgamma / dbeta / fused bias sums, the column-sum kernel, the
// classifier LayerNorm's dgamma / dbeta) write one partial row per workgroup instead and an ordered
// pass sums the rows: every run of a step produces the same bits (bit-exact resume).
bool g_deterministic = [] {
  const char* e = std::getenv("PVR_DETERMINISTIC");
  return e && std::atoi(e) != 0;
}();
void set_deterministic(bool on) { g_deterministic = on; }
bool deterministic() { return g_deterministic; }
// partial-row scratch of the deterministic reductions, one per (device, stream), grown on demand
float* det_scratch(int64_t numel, const torch::TensorOptions& opts) {
  DetWs& d = scratch_map<DetWs>()[scratch_key((int)opts.device().index())];
  if (!d.t.defined() || d.t.numel() < numel) d.t = torch::empty({numel}, opts.dtype(torch::kFloat32));
  return d.t.data_ptr<float>();
}

// C = A . B^T with the given operand layouts; see csrc/gemm.hip for the epilogue contract.
void gemm(torch::Tensor A, bool a_kcontig, torch::Tensor B, bool b_kcontig, torch::Tensor C, int64_t M, int64_t N, int64_t K,
          int64_t epi, c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> resid, c10::optional<torch::Tensor> addend,
          int64_t addend_period, c10::optional<torch::Tensor> aux, int64_t row_group, int64_t row_stride_group,
          int64_t row_offset, c10::optional<torch::Tensor> seed, int64_t seed_offset, double drop_p, int64_t k_split,
          int64_t tile_cfg, c10::optional<torch::Tensor> dbg, c10::optional<torch::Tensor> colsum,
          int64_t epi_staged, int64_t tail_limit, c10::optional<torch::Tensor> reduce_out, bool reduce_acc,
          int64_t drop_row_mul, c10::optional<torch::Tensor> dp_seed, int64_t dp_offset, double dp_p, int64_t dp_rows) {
  pvr::GemmParams p{};
  TORCH_CHECK(drop_row_mul >= 0 && (drop_row_mul == 0 || (tile_cfg == 0 && row_group == 0)) && M * std::max<int64_t>(drop_row_mul, 1) < (int64_t(1) << 31),
              "gemm: drop_row_mul (mask of every drop_row_mul-th row of a larger tensor) needs tile 0 and no row remap");
  p.drop_row_mul = (int)drop_row_mul;
  p.epi_staged = (int)epi_staged;
  if (colsum.has_value() && colsum->defined()) p.colsum = f32_mut(*colsum, "colsum");
  if (dbg.has_value() && dbg->defined()) p.dbg = reinterpret_cast<uint64_t*>(dbg->data_ptr());
  p.drop_scale = 1.f;
  p.M = (int)M; p.N = (int)N; p.K = (int)K;
  p.A = bf(A, "A"); p.lda = ld_of(A, "A"); p.a_kcontig = a_kcontig;
  p.B = bf(B, "B"); p.ldb = ld_of(B, "B"); p.b_kcontig = b_kcontig;
  TORCH_CHECK(N % 8 == 0, "gemm: N must be a multiple of 8");
  if (a_kcontig) TORCH_CHECK(K % 64 == 0, "gemm: K must be a multiple of 64 for a k-contiguous A");
  if (b_kcontig) TORCH_CHECK(K % 64 == 0, "gemm: K must be a multiple of 64 for a k-contiguous B");
  if (a_kcontig) {
    TORCH_CHECK(A.size(0) >= M && A.size(1) >= K, "gemm: A too small");
  } else {
    TORCH_CHECK(A.size(0) >= K && A.size(1) >= M, "gemm: A too small");
  }
  if (b_kcontig) {
    TORCH_CHECK(B.size(0) >= N && B.size(1) >= K, "gemm: B too small");
  } else {
    TORCH_CHECK(B.size(0) >= K && B.size(1) >= N, "gemm: B too small");
  }
  const bool f32out = epi >= 3;
  TORCH_CHECK(C.is_cuda() && C.scalar_type() == (f32out ? torch::kFloat32 : torch::kBFloat16), "gemm: C dtype mismatch for epilogue");
  if (C.dim() == 3) {  // split-K partials [splits, M, N] (EPI_F32_STORE, tile 14)
    TORCH_CHECK(epi == 4 && tile_cfg == 14, "gemm: a 3-D C is the split-K workspace of EPI_F32_STORE / tile 14");
    TORCH_CHECK(C.stride(2) == 1 && C.size(1) >= M && C.size(2) >= N, "gemm: workspace shape");
    const int64_t ks = k_split > 0 ? ((k_split + 63) / 64) * 64 : ((K + 63) / 64) * 64;
    TORCH_CHECK(C.size(0) >= (K + ks - 1) / ks, "gemm: workspace has fewer slices than K splits");
    p.C = C.data_ptr(); p.ldc = C.stride(1); p.split_stride = C.stride(0);
  } else {
    p.C = C.data_ptr(); p.ldc = ld_of(C, "C");
  }
  if (bias.has_value() && bias->defined()) { TORCH_CHECK(bias->numel() >= N && bias->is_contiguous(), "bias"); p.bias = f32(*bias, "bias"); }
  if (resid.has_value() && resid->defined()) { p.resid = bf(*resid, "resid"); p.ld_resid = ld_of(*resid, "resid"); }
  if (addend.has_value() && addend->defined()) { p.addend = f32(*addend, "addend"); p.addend_period = (int)addend_period; TORCH_CHECK(addend_period > 0, "addend_period"); }
  if (aux.has_value() && aux->defined()) { p.aux = const_cast<uint16_t*>(bf(*aux, "aux")); p.ld_aux = ld_of(*aux, "aux"); }
  if (epi == 2) TORCH_CHECK(p.aux != nullptr, "gemm: the dGELU epilogue needs aux");  // GELU: aux optional (inference)
  p.row_group = (int)row_group; p.row_stride_group = (int)row_stride_group; p.row_offset = (int)row_offset;
  set_drop(p, drop_args(seed, seed_offset, drop_p, "gemm"));
  p.k_split_len = k_split > 0 ? (int)(((k_split + 63) / 64) * 64) : (int)(((K + 63) / 64) * 64);
  if (dp_p > 0.0) {
    // drop path of the residual branch: the bf16 residual forward GEMMs on tiles 0, 6, 12, 13
    const pvr::DropSite dp = drop_path_args(dp_seed, dp_offset, dp_p, dp_rows, "gemm: drop_path");
    TORCH_CHECK(epi == 0 && p.resid != nullptr, "gemm: drop_path needs the residual epilogue (EPI_BF16 with resid)");
    TORCH_CHECK(a_kcontig && b_kcontig && row_group == 0 && p.addend == nullptr && p.k_split_len >= K,
                "gemm: drop_path does not combine with row_group / addend / split-K / transposed operands");
    TORCH_CHECK(tile_cfg == 0 || tile_cfg == 6 || tile_cfg == 12 || tile_cfg == 13,
                "gemm: drop_path runs on tiles 0, 6, 12 and 13 (not the wave-specialised tile 15 or the split-K tile 14)");
    TORCH_CHECK(p.seed_ptr == nullptr || p.seed_ptr == dp.seed, "gemm: drop_path and dropout must share the seed tensor");
    TORCH_CHECK(M / dp_rows + 1 < (int64_t(1) << 31), "gemm: drop_path sample index");
    p.seed_ptr = dp.seed;
    p.dp_thr = dp.thr; p.dp_scale = dp.scale; p.dp_seed_offset = dp.offset; p.dp_rows = (int)dp_rows;
  }
  p.epi = (int)epi;
  p.tile_cfg = (int)tile_cfg;
  // tail_limit: -1 = no split tail, 0 = unlimited, n > 0 = at most n workgroups in the split round
  if (epi <= 2 && p.k_split_len >= K && tail_limit >= 0) {
    attach_tail(p, C);
    p.tail_max_units = (int)tail_limit;
    p.tail_min_kt = g_tail_min_kt;
  }
  if (reduce_out.has_value() && reduce_out->defined()) {
    // in-launch reduction of the K splits into reduce_out [M, N] fp32 (GemmParams::sk_*): the
    // ping-pong weight-gradient kernel, every workgroup co-resident
    const torch::Tensor& o = *reduce_out;
    TORCH_CHECK(C.dim() == 3 && epi == 4 && tile_cfg == 14, "gemm: reduce_out needs the split-K workspace form");
    TORCH_CHECK(o.is_cuda() && o.scalar_type() == torch::kFloat32 && o.dim() == 2 && o.stride(1) == 1 && o.size(0) >= M && o.size(1) >= N &&
                    o.stride(0) % 4 == 0 && reinterpret_cast<uintptr_t>(o.data_ptr()) % 16 == 0,
                "gemm: reduce_out must be a 16-B aligned fp32 [M, N] tensor with unit column stride");
    const int64_t splits = (K + p.k_split_len - 1) / p.k_split_len;
    const int64_t tiles = ((M + 255) / 256) * ((N + 255) / 256);
    TORCH_CHECK(N % 4 == 0 && tiles <= g_sk_tiles && tiles * splits <= num_cus(), "gemm: reduce_out: too many workgroups to be co-resident");
    TORCH_CHECK(p.split_stride * 4 * (2 * splits + 16) < (int64_t(1) << 32) && M * p.ldc * 4 < (int64_t(1) << 31),
                "gemm: reduce_out: workspace too large for 32-bit buffer offsets");
    torch::Tensor& cnt = splitk_counters(o);
    p.sk_out = o.data_ptr<float>();
    p.sk_ldo = o.stride(0);
    p.sk_acc = reduce_acc ? 1 : 0;
    p.sk_cnt = reinterpret_cast<unsigned*>(cnt.data_ptr<int32_t>());
    p.sk_cnt_tiles = g_sk_tiles;
  }
  check(pvr_gemm(&p, stream()), "gemm");
}

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w, torch::Tensor b, double eps, int64_t rows,
                                         int64_t x_row_stride) {
  const int64_t D = w.numel();
  auto y = torch::empty({rows, D}, x.options());
  auto mean = torch::empty({rows}, x.options().dtype(torch::kFloat32));
  auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat32));
  TORCH_CHECK(x.stride(-1) == 1, "layernorm: x last dim must be contiguous");
  check(pvr_layernorm_fwd(bf(x, "x"), x_row_stride, f32(w, "w"), f32(b, "b"), bf_mut(y, "y"), D, f32_mut(mean, "mean"),
                          f32_mut(rstd, "rstd"), (int)rows, (int)D, (float)eps, stream()),
        "layernorm_fwd");
  return {y, mean, rstd};
}

// layernorm_fwd + the output's e4m3 copy q_out [rows][D] (uint8) quantized with *q_scale, amax
// recorded into *q_amax (int32 float bits): the fp8 forward's quantize pass folded into the LayerNorm
std::vector<torch::Tensor> layernorm_fwd_q8(torch::Tensor x, torch::Tensor w, torch::Tensor b, double eps, int64_t rows,
                                            int64_t x_row_stride, torch::Tensor q_out, torch::Tensor q_scale, torch::Tensor q_amax,
                                            bool skip_y) {
  const int64_t D = w.numel();
  auto y = torch::empty({rows, D}, x.options());
  auto mean = torch::empty({rows}, x.options().dtype(torch::kFloat32));
  auto rstd = torch::empty({rows}, x.options().dtype(torch::kFloat32));
  TORCH_CHECK(x.stride(-1) == 1, "layernorm: x last dim must be contiguous");
  TORCH_CHECK(q_out.defined(), "layernorm_fwd_q8: q_out is required");
  const pvr::Fp8Copy q = fp8_copy(q_out, q_scale, q_amax, 0, rows, D, 8, "layernorm_fwd_q8");
  // skip_y: only the e4m3 copy is consumed (the bf16 y stays allocated, unwritten)
  check(pvr_layernorm_fwd_q8(bf(x, "x"), x_row_stride, f32(w, "w"), f32(b, "b"), skip_y ? nullptr : bf_mut(y, "y"), D, q,
                             f32_mut(mean, "mean"), f32_mut(rstd, "rstd"), (int)rows, (int)D, (float)eps, stream()),
        "layernorm_fwd_q8");
  return {y, mean, rstd};
}

// dz (optional, needs drop_p > 0): dropout backward of the layer that produced x's residual stream,
// dz = mask(seed + seed_offset) * scale * dx; dsum then receives the column sums of dz instead of dx.
void layernorm_bwd(torch::Tensor dy, int64_t dy_stride, torch::Tensor x, int64_t x_stride, torch::Tensor mean, torch::Tensor rstd,
                   torch::Tensor w, c10::optional<torch::Tensor> dres, int64_t dres_stride, torch::Tensor dx, int64_t dx_stride,
                   c10::optional<torch::Tensor> dw, c10::optional<torch::Tensor> db, int64_t rows,
                   c10::optional<torch::Tensor> dsum, c10::optional<torch::Tensor> dz, c10::optional<torch::Tensor> seed,
                   int64_t seed_offset, double drop_p, c10::optional<torch::Tensor> q_out,
                   c10::optional<torch::Tensor> q_scale, c10::optional<torch::Tensor> q_amax, bool dz_nostore,
                   int64_t q_fmt, int64_t dres_every, c10::optional<torch::Tensor> dp_seed, int64_t dp_offset, double dp_p,
                   int64_t dp_rows) {
  const int64_t D = w.numel();
  pvr::LnBwdParams p{};
  TORCH_CHECK(dres_every >= 0, "layernorm_bwd: dres_every >= 0");
  if (dres_every > 1) {
    TORCH_CHECK(dres.has_value() && dres->defined() && dres->numel() >= ((rows + dres_every - 1) / dres_every - 1) * dres_stride + D &&
                    !(q_out.has_value() && q_out->defined()),
                "layernorm_bwd: dres_every needs a compact dres [ceil(rows / dres_every)][D] and no fp8 copy");
  }
  p.dres_every = (int)dres_every;
  p.dy = bf(dy, "dy"); p.dy_stride = dy_stride;
  p.x = bf(x, "x"); p.x_stride = x_stride;
  p.mean = f32(mean, "mean"); p.rstd = f32(rstd, "rstd"); p.w = f32(w, "w");
  p.dres = opt_ptr<const uint16_t>(dres); p.dres_stride = dres_stride;
  p.dx = bf_mut(dx, "dx"); p.dx_stride = dx_stride;
  p.dw = opt_ptr<float>(dw); p.db = opt_ptr<float>(db); p.dsum = opt_ptr<float>(dsum);
  const bool has_dz = dz.has_value() && dz->defined();
  if (has_dz) {
    TORCH_CHECK(drop_p > 0.0 || dp_p > 0.0, "layernorm_bwd: dz is the dropout / drop_path backward, it needs drop_p > 0 or a drop_path rate > 0");
    p.dz = const_cast<uint16_t*>(bf(*dz, "dz"));
    p.dz_stride = ld_of(*dz, "dz");
  }
  p.drop = drop_args(seed, seed_offset, has_dz ? drop_p : 0.0, "layernorm_bwd");
  if (dp_p > 0.0) {
    TORCH_CHECK(has_dz, "layernorm_bwd: drop_path scales the dz output, it needs dz");
    TORCH_CHECK(!(q_out.has_value() && q_out->defined()), "layernorm_bwd: drop_path does not combine with the fp8 copy (q_out)");
    p.dpath = drop_path_args(dp_seed, dp_offset, dp_p, dp_rows, "layernorm_bwd: drop_path");
    p.dp_rows = (int)dp_rows;
  }
  p.dz_nostore = dz_nostore ? 1 : 0;
  // optional e5m2 copy of the last-written gradient (dz if given, else dx) with a delayed scale
  // and an amax record: the producer-side quantization for the next fp8 dgrad GEMM
  p.q = fp8_copy(q_out, q_scale, q_amax, q_fmt, rows, D, 8, "layernorm_bwd");
  p.rows = (int)rows; p.D = (int)D;
  if (g_deterministic && (p.dw || p.db || p.dsum))
    p.part = det_scratch((int64_t)pvr_layernorm_bwd_blocks((int)rows, (int)D) * 3 * D, x.options());
  check(pvr_layernorm_bwd(&p, stream()), "layernorm_bwd");
}

// out (+)= ws.sum(0) for a split-K workspace ws [S, rows, cols] (out: contiguous [rows, cols])
// out (+)= ws[:S].sum(0) for ws [S, rows, wcols]; out [rows, ocols] contiguous with ocols <= wcols
// (the leading columns of each workspace row: a K-padded weight gradient reduced into the unpadded one)
void splitk_reduce(torch::Tensor ws, int64_t S, torch::Tensor out, bool accumulate) {
  TORCH_CHECK(ws.dim() == 3 && ws.size(0) >= S && S >= 1, "splitk_reduce: ws must be [S, rows, cols]");
  TORCH_CHECK(out.is_contiguous() && ws.stride(2) == 1 && ws.stride(1) == ws.size(2), "splitk_reduce: layouts");
  const int64_t rows = ws.size(1), wcols = ws.size(2);
  TORCH_CHECK(out.numel() % rows == 0, "splitk_reduce: out must hold [rows, ocols]");
  const int64_t ocols = out.numel() / rows;
  TORCH_CHECK(ocols <= wcols && ocols % 4 == 0 && wcols % 4 == 0, "splitk_reduce: out columns must be a 4-aligned prefix of ws columns");
  check(pvr_splitk_reduce(f32(ws, "ws"), (int)S, ws.stride(0), f32_mut(out, "out"), out.numel(), (int)ocols, (int)wcols,
                          accumulate ? 1 : 0, stream()),
        "splitk_reduce");
}

// dst [rows, ld] bf16 = src [rows, cols] zero-padded on the right (cols, ld % 4 == 0)
void pad_cols_bf16(torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(src.is_contiguous() && dst.is_contiguous() && src.dim() == 2 && dst.dim() == 2 && src.size(0) == dst.size(0) &&
                  src.size(1) <= dst.size(1) && src.size(1) % 4 == 0 && dst.size(1) % 4 == 0,
              "pad_cols_bf16: src [rows, cols], dst [rows, ld >= cols], contiguous, 4-aligned");
  check(pvr_pad_cols_bf16(bf(src, "src"), (int)src.size(0), (int)src.size(1), bf_mut(dst, "dst"), (int)dst.size(1), stream()),
        "pad_cols_bf16");
}

// out = bf16(epilogue(ws.sum(0))) for a split-K workspace ws [S, M, N]: + bias, GELU (inference: no
// derivative), + resid (the small-M forward GEMM's reduction pass)
void splitk_epilogue(torch::Tensor ws, int64_t S, torch::Tensor out, c10::optional<torch::Tensor> bias,
                     c10::optional<torch::Tensor> resid, bool gelu) {
  TORCH_CHECK(ws.dim() == 3 && ws.size(0) >= S && S >= 1 && ws.stride(2) == 1 && ws.stride(1) == ws.size(2),
              "splitk_epilogue: ws must be [S, M, N] with contiguous rows");
  const int64_t M = ws.size(1), N = ws.size(2);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == N && N % 4 == 0, "splitk_epilogue: out shape");
  const int64_t ldc = ld_of(out, "out");
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->numel() >= N && bias->is_contiguous(), "splitk_epilogue: bias");
    bp = f32(*bias, "bias");
  }
  const uint16_t* rp = nullptr;
  int64_t ldr = 0;
  if (resid.has_value() && resid->defined()) {
    TORCH_CHECK(resid->dim() == 2 && resid->size(0) >= M && resid->size(1) >= N, "splitk_epilogue: resid must cover [M, N]");
    rp = bf(*resid, "resid");
    ldr = ld_of(*resid, "resid");
  }
  check(pvr_splitk_epilogue(f32(ws, "ws"), (int)S, ws.stride(0), (int)M, (int)N, bp, rp, ldr, gelu ? 1 : 0, bf_mut(out, "out"), ldc,
                            stream()),
        "splitk_epilogue");
}

void cast_f32_bf16(torch::Tensor in, torch::Tensor out) {
  TORCH_CHECK(in.is_contiguous() && out.is_contiguous() && in.numel() == out.numel(), "cast: shape/contiguity");
  TORCH_CHECK(in.device() == out.device() && reinterpret_cast<uintptr_t>(in.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(out.data_ptr()) % 8 == 0,
              "cast: in (16-byte aligned) and out (8-byte aligned) on one GPU");
  check(pvr_cast_f32_bf16(f32(in, "in"), bf_mut(out, "out"), in.numel(), stream()), "cast_f32_bf16");
}

void transpose_batched(torch::Tensor src, torch::Tensor dst, torch::Tensor meta, int64_t total_tiles) {
  TORCH_CHECK(meta.scalar_type() == torch::kInt64 && meta.is_cuda() && meta.dim() == 2 && meta.size(1) == 5, "meta");
  check(pvr_transpose_batched(bf(src, "src"), bf_mut(dst, "dst"), meta.data_ptr<int64_t>(), (int)meta.size(0), (int)total_tiles,
                              stream()),
        "transpose_batched");
}

void colsum(torch::Tensor dy, int64_t rows, int64_t N, c10::optional<torch::Tensor> db, c10::optional<torch::Tensor> dz,
            c10::optional<torch::Tensor> seed, int64_t seed_offset, double drop_p, c10::optional<torch::Tensor> q_out,
            c10::optional<torch::Tensor> q_scale, c10::optional<torch::Tensor> q_amax, int64_t q_fmt, int64_t row_mul,
            c10::optional<torch::Tensor> dp_seed, int64_t dp_offset, double dp_p, int64_t dp_rows) {
  TORCH_CHECK(row_mul >= 1 && rows * row_mul < (int64_t(1) << 31), "colsum: row_mul >= 1 and rows * row_mul < 2^31");
  const pvr::DropSite d = drop_args(seed, seed_offset, drop_p, "colsum");
  pvr::DropSite dp;
  if (dp_p > 0.0) {
    TORCH_CHECK(!(q_out.has_value() && q_out->defined()), "colsum: drop_path does not combine with the fp8 copy (q_out)");
    dp = drop_path_args(dp_seed, dp_offset, dp_p, dp_rows, "colsum: drop_path");
  }
  int64_t ldz = 0;
  uint16_t* dzp = nullptr;
  if (dz.has_value() && dz->defined()) { dzp = const_cast<uint16_t*>(bf(*dz, "dz")); ldz = ld_of(*dz, "dz"); }
  // optional fp8 copy (q_fmt 1 e5m2, 0 e4m3) of the (masked) gradient + amax record (the fp8 dgrad operand)
  const pvr::Fp8Copy q = fp8_copy(q_out, q_scale, q_amax, q_fmt, rows, N, 8, "colsum");
  check(pvr_colsum(bf(dy, "dy"), ld_of(dy, "dy"), (int)rows, (int)N, opt_ptr<float>(db), dzp, ldz, d, q,
                   g_deterministic && opt_ptr<float>(db) ? det_scratch((int64_t)pvr_colsum_part_rows((int)rows) * N, dy.options()) : nullptr,
                   (int)row_mul, dp, (int)std::max<int64_t>(dp_rows, 1), stream()),
        "colsum");
}

// s [B] float32: the drop-path scale vector of site (seed + site_offset) at rate p, 0 or 65536 / (65536 - thr)
// per sample, exactly the draws the fused kernels make (the torch fallback's and the tests' replay)
torch::Tensor drop_path_scale(torch::Tensor seed, int64_t site_offset, double p, int64_t B) {
  TORCH_CHECK(B >= 0 && B < (int64_t(1) << 31), "drop_path_scale: B");
  auto out = torch::ones({B}, seed.options().dtype(torch::kFloat32));
  if (p <= 0.0 || B == 0) return out;
  const pvr::DropSite dp = drop_path_args(seed, site_offset, p, 1, "drop_path_scale");
  check(pvr_drop_path_scale(dp, out.data_ptr<float>(), (int)B, stream()), "drop_path_scale");
  return out;
}

// A batch-mix plan for the patchify kernels (csrc/kernels.h MixRow): `mix` int32 [B, 8] on the image's
// device, validated here on the host so that no kernel ever sees a partner outside [0, B) or a box
// outside the H x W output. `host` is the CPU tensor the device copy was uploaded from (MixPlan keeps
// it); without it the device tensor is read back, which synchronises.
const pvr::MixRow* mix_rows(const c10::optional<torch::Tensor>& mix, const c10::optional<torch::Tensor>& host, int64_t B, int64_t H,
                            int64_t W, const torch::Tensor& img, const char* what) {
  if (!mix.has_value() || !mix->defined()) {
    TORCH_CHECK(!host.has_value() || !host->defined(), what, ": mix_host without mix");
    return nullptr;
  }
  TORCH_CHECK(mix->is_cuda() && mix->device() == img.device(), what, ": mix must be on the image's device");
  TORCH_CHECK(mix->scalar_type() == torch::kInt32 && mix->dim() == 2 && mix->size(0) == B && mix->size(1) == 8 && mix->is_contiguous(),
              what, ": mix must be contiguous int32 [", B, ", 8]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(mix->data_ptr()) % 16 == 0, what, ": mix must be 16-byte aligned");
  torch::Tensor h;
  if (host.has_value() && host->defined()) {
    TORCH_CHECK(!host->is_cuda() && host->scalar_type() == torch::kInt32 && host->dim() == 2 && host->size(0) == B &&
                    host->size(1) == 8 && host->is_contiguous(),
                what, ": mix_host must be a contiguous CPU int32 [", B, ", 8] tensor");
    h = *host;
  } else {
    h = mix->cpu();
  }
  const auto* rows = reinterpret_cast<const pvr::MixRow*>(h.data_ptr());
  for (int64_t b = 0; b < B; ++b) {
    const pvr::MixRow& r = rows[b];
    TORCH_CHECK(r.partner >= 0 && r.partner < B, what, ": mix row ", b, " has partner ", r.partner, " outside [0, ", B, ")");
    TORCH_CHECK(r.lam >= 0.f && r.lam <= 1.f, what, ": mix row ", b, " has lam ", r.lam, " outside [0, 1]");
    TORCH_CHECK(r.bx0 >= 0 && r.bx0 <= r.bx1 && r.bx1 <= W && r.by0 >= 0 && r.by0 <= r.by1 && r.by1 <= H, what, ": mix row ", b,
                " has box (", r.bx0, ", ", r.by0, ", ", r.bx1, ", ", r.by1, ") outside the ", H, "x", W, " image");
  }
  return reinterpret_cast<const pvr::MixRow*>(mix->data_ptr());
}

// A random-erasing plan for the patchify kernels (csrc/kernels.h EraseRow / EraseArgs): `erase` int32 [B, 4]
// on the image's device, validated here on the host like a mix plan (`host`: the CPU tensor it was
// uploaded from, data/random_erasing.py ErasePlan; without it the device tensor is read back, which
// synchronises), before any kernel runs. mode: "const" (value: one float per channel, or one for all) or
// "pixel" (seed: the step's int64 device counter, offset: the site's offset).
pvr::EraseArgs erase_args(const c10::optional<torch::Tensor>& erase, const c10::optional<torch::Tensor>& host, const std::string& mode,
                          const std::vector<double>& value, const c10::optional<torch::Tensor>& seed, int64_t offset, int64_t B,
                          int64_t C, int64_t H, int64_t W, const torch::Tensor& img, const char* what) {
  pvr::EraseArgs e;
  if (!erase.has_value() || !erase->defined()) {
    TORCH_CHECK(!host.has_value() || !host->defined(), what, ": erase_host without erase");
    return e;
  }
  TORCH_CHECK(erase->is_cuda() && erase->device() == img.device(), what, ": erase must be on the image's device");
  TORCH_CHECK(erase->scalar_type() == torch::kInt32 && erase->dim() == 2 && erase->size(0) == B && erase->size(1) == 4 &&
                  erase->is_contiguous(),
              what, ": erase must be contiguous int32 [", B, ", 4]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(erase->data_ptr()) % 16 == 0, what, ": erase must be 16-byte aligned");
  TORCH_CHECK(C >= 1 && C <= 4, what, ": erasing takes 1..4 channels, got ", C);
  TORCH_CHECK(B * C * H * W < (int64_t(1) << 62), what, ": erase: too many elements");
  torch::Tensor h;
  if (host.has_value() && host->defined()) {
    TORCH_CHECK(!host->is_cuda() && host->scalar_type() == torch::kInt32 && host->dim() == 2 && host->size(0) == B &&
                    host->size(1) == 4 && host->is_contiguous(),
                what, ": erase_host must be a contiguous CPU int32 [", B, ", 4] tensor");
    h = *host;
  } else {
    h = erase->cpu();
  }
  const auto* rows = reinterpret_cast<const pvr::EraseRow*>(h.data_ptr());
  for (int64_t b = 0; b < B; ++b) {
    const pvr::EraseRow& r = rows[b];
    TORCH_CHECK(r.x0 >= 0 && r.x0 <= r.x1 && r.x1 <= W && r.y0 >= 0 && r.y0 <= r.y1 && r.y1 <= H, what, ": erase row ", b,
                " has box (", r.x0, ", ", r.y0, ", ", r.x1, ", ", r.y1, ") outside the ", H, "x", W, " image");
  }
  if (mode == "pixel") {
    TORCH_CHECK(seed.has_value() && seed->defined(), what, ": erase mode \"pixel\" needs erase_seed, the int64 device counter");
    TORCH_CHECK(seed->is_cuda() && seed->device() == img.device() && seed->scalar_type() == torch::kInt64 && seed->numel() >= 1,
                what, ": erase_seed must be an int64 tensor on the image's device");
    e.mode = pvr::ERASE_PIXEL;
    e.seed = reinterpret_cast<const uint64_t*>(seed->data_ptr());
    e.offset = (uint64_t)offset;
  } else {
    TORCH_CHECK(mode == "const", what, ": erase_mode must be \"pixel\" or \"const\", got \"", mode, "\"");
    TORCH_CHECK(value.size() == 1 || (int64_t)value.size() == C, what, ": erase_value needs one value, or one per channel");
    for (int64_t c = 0; c < C; ++c) e.value[c] = (float)value[value.size() == 1 ? 0 : c];
  }
  e.rows = reinterpret_cast<const pvr::EraseRow*>(erase->data_ptr());
  return e;
}

// The "pixel" fill of random erasing for every element of a [B, C, H, W] model image at site `site_offset`
// of the counter value *seed (csrc/elementwise.hip erase_normal, the function the patchify kernels call):
// diagnostics, and the tests' and the reference path's replay of the kernels' noise.
torch::Tensor erase_noise(torch::Tensor seed, int64_t site_offset, int64_t B, int64_t C, int64_t H, int64_t W) {
  TORCH_CHECK(seed.is_cuda() && seed.scalar_type() == torch::kInt64 && seed.numel() >= 1,
              "erase_noise: seed must be an int64 tensor on the GPU");
  TORCH_CHECK(B >= 0 && C >= 0 && H >= 0 && W >= 0 && B < (1ll << 31) && C < (1ll << 31) && H < (1ll << 31) && W < (1ll << 31),
              "erase_noise: bad shape");
  auto out = torch::empty({B, C, H, W}, seed.options().dtype(torch::kFloat32));
  check(pvr_erase_noise(reinterpret_cast<const uint64_t*>(seed.data_ptr()), (uint64_t)site_offset, out.data_ptr<float>(), out.numel(),
                        stream()),
        "erase_noise");
  return out;
}

// Patch dropout's keep table (csrc/elementwise.hip patch_keep_kernel): (keep int32 [B, n_keep], inv int32
// [B, n_p]) of the site `site_offset` at the counter value *seed. The fused forward's draw, and the
// tests' and the reference path's replay of it.
std::tuple<torch::Tensor, torch::Tensor> patch_keep_table(torch::Tensor seed, int64_t site_offset, int64_t B, int64_t n_p,
                                                          int64_t n_keep) {
  TORCH_CHECK(seed.is_cuda() && seed.scalar_type() == torch::kInt64 && seed.numel() >= 1,
              "patch_keep_table: seed must be an int64 tensor on the GPU");
  TORCH_CHECK(n_p >= 1 && n_p <= 4096, "patch_keep_table: n_p must be in [1, 4096], got ", n_p);
  TORCH_CHECK(n_keep >= 1 && n_keep <= n_p, "patch_keep_table: n_keep must be in [1, n_p = ", n_p, "], got ", n_keep);
  TORCH_CHECK(B >= 0 && B * n_p < (int64_t(1) << 32), "patch_keep_table: B * n_p must be below 2^32");
  auto keep = torch::empty({B, n_keep}, seed.options().dtype(torch::kInt32));
  auto inv = torch::empty({B, n_p}, seed.options().dtype(torch::kInt32));
  check(pvr_patch_keep(reinterpret_cast<const uint64_t*>(seed.data_ptr()), (uint64_t)site_offset, (int)B, (int)n_p, (int)n_keep,
                       keep.data_ptr<int>(), inv.data_ptr<int>(), stream()),
        "patch_keep_table");
  return std::make_tuple(keep, inv);
}

// A keep table as a kernel argument: contiguous int32 [B, n_keep] on `like`'s device, 1 <= n_keep <= n_p
const int* keep_rows(const c10::optional<torch::Tensor>& keep, int64_t B, int64_t n_p, const torch::Tensor& like, int64_t* n_keep,
                     const char* what) {
  *n_keep = 0;
  if (!keep.has_value() || !keep->defined()) return nullptr;
  TORCH_CHECK(keep->is_cuda() && keep->device() == like.device() && keep->scalar_type() == torch::kInt32 && keep->dim() == 2 &&
                  keep->is_contiguous() && keep->size(0) == B && keep->size(1) >= 1 && keep->size(1) <= n_p,
              what, ": keep must be contiguous int32 [", B, ", 1 .. ", n_p, "] on the input's device");
  *n_keep = keep->size(1);
  return keep->data_ptr<int>();
}

// the embedding GEMM's position addend under patch dropout (csrc/elementwise.hip pos_gather_kernel)
torch::Tensor pos_gather(torch::Tensor pos, torch::Tensor keep) {
  TORCH_CHECK(pos.dim() == 2 && pos.is_contiguous() && pos.size(0) >= 2 && pos.size(1) % 4 == 0, "pos_gather: pos must be contiguous [n_p + 1, D], D % 4 == 0");
  const int64_t n_p = pos.size(0) - 1, D = pos.size(1);
  TORCH_CHECK(keep.dim() == 2, "pos_gather: keep must be [B, n_keep]");
  const int64_t B = keep.size(0);
  int64_t n_keep = 0;
  const int* kp = keep_rows(keep, B, n_p, pos, &n_keep, "pos_gather");
  TORCH_CHECK(B * (n_keep + 1) < (int64_t(1) << 31), "pos_gather: too many rows");
  auto out = torch::empty({B * (n_keep + 1), D}, pos.options());
  check(pvr_pos_gather(f32(pos, "pos"), kp, out.data_ptr<float>(), (int)B, (int)n_p, (int)n_keep, (int)D, stream()), "pos_gather");
  return out;
}

void im2col(torch::Tensor img, torch::Tensor out, int64_t P, int64_t Kp, c10::optional<torch::Tensor> mix,
            c10::optional<torch::Tensor> mix_host, c10::optional<torch::Tensor> keep, c10::optional<torch::Tensor> erase,
            c10::optional<torch::Tensor> erase_host, std::string erase_mode, std::vector<double> erase_value,
            c10::optional<torch::Tensor> erase_seed, int64_t erase_offset) {
  TORCH_CHECK(img.is_contiguous() && img.dim() == 4, "im2col: img must be contiguous NCHW");
  const pvr::MixRow* mp = mix_rows(mix, mix_host, img.size(0), img.size(2), img.size(3), img, "im2col");
  const pvr::EraseArgs ea = erase_args(erase, erase_host, erase_mode, erase_value, erase_seed, erase_offset, img.size(0), img.size(1),
                                       img.size(2), img.size(3), img, "im2col");
  int64_t n_keep = 0;
  const int* kp = nullptr;
  if (keep.has_value() && keep->defined()) {  // (the plain call keeps its checks, as with a plan below)
    TORCH_CHECK(P > 0, "im2col: patch size");
    kp = keep_rows(keep, img.size(0), (img.size(2) / P) * (img.size(3) / P), img, &n_keep, "im2col");
  }
  if (mp || kp || ea.rows) {  // the plain call keeps its checks; a plan adds those that keep the second read in bounds
    const int64_t rows = P > 0 ? img.size(0) * (kp ? n_keep : (img.size(2) / P) * (img.size(3) / P)) : -1;
    TORCH_CHECK(img.is_cuda() && P > 0 && img.size(2) % P == 0 && img.size(3) % P == 0 && Kp % 8 == 0 &&
                    Kp >= img.size(1) * P * P,
                "im2col: the image must be a GPU tensor whose sides are multiples of the patch size, Kp a multiple of 8 >= C*P*P");
    TORCH_CHECK(out.is_cuda() && out.device() == img.device() && out.is_contiguous() && out.dim() == 2 && out.size(0) == rows &&
                    out.size(1) == Kp,
                "im2col: out must be contiguous bf16 [", rows, ", ", Kp, "] on the image's device");
  }
  check(pvr_im2col(f32(img, "img"), bf_mut(out, "out"), (int)img.size(0), (int)img.size(1), (int)img.size(2), (int)img.size(3),
                   (int)P, (int)Kp, mp, kp, (int)n_keep, ea, stream()),
        "im2col");
}

// uint8 [B, C <= 4, Hs, Ws] image (any strides: contiguous NCHW, channels_last, views) -> the bf16
// patch rows of im2col, normalised ((p / 255 - mean[c]) / std[c]) and, with geom [B, 4] float32,
// cropped / resized / flipped per sample (csrc/elementwise.hip im2col_u8_kernel). Returns 1 when
// the 8-byte-load path ran, 0 for the per-element path (decided here from data_ptr and strides).
int64_t im2col_u8(torch::Tensor img, torch::Tensor out, std::vector<double> mean, std::vector<double> stdv,
                  c10::optional<torch::Tensor> geom, int64_t H, int64_t W, int64_t P, int64_t Kp, c10::optional<torch::Tensor> mix,
                  c10::optional<torch::Tensor> mix_host, c10::optional<torch::Tensor> keep, c10::optional<torch::Tensor> erase,
                  c10::optional<torch::Tensor> erase_host, std::string erase_mode, std::vector<double> erase_value,
                  c10::optional<torch::Tensor> erase_seed, int64_t erase_offset) {
  TORCH_CHECK(img.is_cuda() && img.scalar_type() == torch::kUInt8, "im2col_u8: img must be a uint8 GPU tensor, got ",
              img.scalar_type(), " on ", img.device());
  TORCH_CHECK(img.dim() == 4, "im2col_u8: img must be [B, C, Hs, Ws], got ", img.dim(), " dims");
  const int64_t B = img.size(0), C = img.size(1), Hs = img.size(2), Ws = img.size(3);
  TORCH_CHECK(C >= 1 && C <= 4, "im2col_u8: 1..4 channels, got ", C);
  TORCH_CHECK((int64_t)mean.size() == C && (int64_t)stdv.size() == C, "im2col_u8: mean / std need one value per channel");
  for (double sd : stdv) TORCH_CHECK(sd != 0.0, "im2col_u8: std must be non-zero");
  TORCH_CHECK(P > 0 && H > 0 && W > 0 && H % P == 0 && W % P == 0, "im2col_u8: output ", H, "x", W,
              " must be a positive multiple of the patch size ", P);
  TORCH_CHECK(Hs >= 1 && Ws >= 1 && Hs < (1 << 24) && Ws < (1 << 24), "im2col_u8: bad source size ", Hs, "x", Ws);
  int64_t n_keep = 0;
  const int* kp = keep_rows(keep, B, (H / P) * (W / P), img, &n_keep, "im2col_u8");
  const int64_t rows = B * (kp ? n_keep : (H / P) * (W / P));
  TORCH_CHECK(Kp % 8 == 0 && Kp >= C * P * P, "im2col_u8: Kp must be a multiple of 8 and >= C*P*P");
  TORCH_CHECK(B < (1ll << 31) && rows < (1ll << 31) && Kp < (1ll << 31), "im2col_u8: sizes exceed 32 bits");
  TORCH_CHECK(out.is_cuda() && out.device() == img.device() && out.is_contiguous() && out.dim() == 2 && out.size(0) == rows &&
                  out.size(1) == Kp,
              "im2col_u8: out must be contiguous bf16 [", rows, ", ", Kp, "] on the image's device");
  const float* gp = nullptr;
  if (geom.has_value() && geom->defined()) {
    TORCH_CHECK(geom->is_cuda() && geom->device() == img.device(), "im2col_u8: geom must be on the image's device");
    TORCH_CHECK(geom->scalar_type() == torch::kFloat32 && geom->dim() == 2 && geom->size(0) == B && geom->size(1) == 4 &&
                    geom->is_contiguous(),
                "im2col_u8: geom must be contiguous float32 [", B, ", 4]");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(geom->data_ptr()) % 16 == 0, "im2col_u8: geom must be 16-byte aligned");
    gp = geom->data_ptr<float>();
  } else {
    TORCH_CHECK(Hs == H && Ws == W, "im2col_u8: a ", Hs, "x", Ws, " source needs geom to produce ", H, "x", W);
  }
  const pvr::MixRow* mp = mix_rows(mix, mix_host, B, H, W, img, "im2col_u8");
  const pvr::EraseArgs ea = erase_args(erase, erase_host, erase_mode, erase_value, erase_seed, erase_offset, B, C, H, W, img, "im2col_u8");
  const int64_t sb = img.stride(0), sc = img.stride(1), sy = img.stride(2), sx = img.stride(3);
  TORCH_CHECK(sb >= 0 && sc >= 0 && sy >= 0 && sx >= 0, "im2col_u8: negative strides");
  const uint8_t* ip = img.data_ptr<uint8_t>();
  const int vec = !gp && sx == 1 && P % 8 == 0 && reinterpret_cast<uintptr_t>(ip) % 8 == 0 && sb % 8 == 0 && sc % 8 == 0 && sy % 8 == 0;
  float m[4], sd[4];
  for (int64_t c = 0; c < C; ++c) {
    m[c] = (float)mean[c];
    sd[c] = (float)stdv[c];
  }
  check(pvr_im2col_u8(ip, sb, sc, sy, sx, m, sd, gp, bf_mut(out, "out"), (int)B, (int)C, (int)Hs, (int)Ws, (int)H, (int)W, (int)P,
                      (int)Kp, vec, mp, kp, (int)n_keep, ea, stream()),
        "im2col_u8");
  return vec;
}

// Colour augmentation of a raw uint8 [B, 3, Hs, Ws] batch (csrc/color.hip; data/color_augment.py ColorPlan):
// returns a new batch (the layout of `img` when that is dense, contiguous otherwise); `img` is untouched.
// `plan`: float32 [B, 20] ColorRow table on the image's device; `host`: the CPU tensor it was uploaded from
// (without it the device table is read back, which synchronises). Everything is validated on the host copy
// before any launch.
torch::Tensor color_u8(torch::Tensor img, torch::Tensor plan, c10::optional<torch::Tensor> host) {
  TORCH_CHECK(img.is_cuda() && img.scalar_type() == torch::kUInt8, "color_u8: img must be a uint8 GPU tensor, got ", img.scalar_type(),
              " on ", img.device());
  TORCH_CHECK(img.dim() == 4, "color_u8: img must be [B, 3, Hs, Ws], got ", img.dim(), " dims");
  const int64_t B = img.size(0), C = img.size(1), Hs = img.size(2), Ws = img.size(3);
  TORCH_CHECK(C == 3, "color_u8: colour augmentation takes 3 channels, got ", C);
  TORCH_CHECK(Hs >= 1 && Ws >= 1 && Hs * Ws <= (int64_t(1) << 24), "color_u8: bad source size ", Hs, "x", Ws,
              " (at most 2^24 pixels: the luma sum is 32 bits wide)");
  TORCH_CHECK(B < (1ll << 31), "color_u8: sizes exceed 32 bits");
  constexpr int64_t RW = sizeof(pvr::ColorRow) / 4;
  TORCH_CHECK(plan.is_cuda() && plan.device() == img.device(), "color_u8: plan must be on the image's device");
  TORCH_CHECK(plan.scalar_type() == torch::kFloat32 && plan.dim() == 2 && plan.size(0) == B && plan.size(1) == RW && plan.is_contiguous(),
              "color_u8: plan must be contiguous float32 [", B, ", ", RW, "], got [", plan.size(0), ", ", plan.dim() == 2 ? plan.size(1) : -1,
              "]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(plan.data_ptr()) % 16 == 0, "color_u8: plan must be 16-byte aligned");
  torch::Tensor h;
  if (host.has_value() && host->defined()) {
    TORCH_CHECK(!host->is_cuda() && host->scalar_type() == torch::kFloat32 && host->dim() == 2 && host->size(0) == B &&
                    host->size(1) == RW && host->is_contiguous(),
                "color_u8: plan_host must be a contiguous CPU float32 [", B, ", ", RW, "] tensor");
    h = *host;
  } else {
    h = plan.cpu();
  }
  const auto* rows = reinterpret_cast<const pvr::ColorRow*>(h.data_ptr());
  bool any_blur = false, any_sum = false;
  for (int64_t b = 0; b < B; ++b) {
    const pvr::ColorRow& r = rows[b];
    TORCH_CHECK(r.op >= pvr::COLOR_NONE && r.op <= pvr::COLOR_BLUR, "color_u8: row ", b, " has op ", r.op, " outside 0..3");
    TORCH_CHECK(r.order >= 0 && r.order < 6, "color_u8: row ", b, " has order ", r.order, " outside 0..5");
    for (float f : {r.fb, r.fc, r.fs})
      TORCH_CHECK(std::isfinite(f) && f >= 0.f, "color_u8: row ", b, " has a jitter factor ", f, " that is not finite and >= 0");
    if (r.op == pvr::COLOR_BLUR) {
      TORCH_CHECK(r.sigma > 0.f && r.sigma <= pvr::COLOR_SIGMA_MAX, "color_u8: row ", b, " has sigma ", r.sigma, " outside (0, ",
                  pvr::COLOR_SIGMA_MAX, "]");
      double sum = 0.0;
      for (float w : r.w) {
        TORCH_CHECK(std::isfinite(w) && w >= 0.f && w <= 1.f, "color_u8: row ", b, " has a blur weight ", w, " outside [0, 1]");
        sum += w;
      }
      TORCH_CHECK(std::fabs(sum - 1.0) < 1e-5, "color_u8: row ", b, "'s blur weights sum to ", sum, ", not 1");
      any_blur = true;
    }
    any_sum = any_sum || r.fc != 1.f;
  }
  auto out = torch::empty_like(img);  // dense inputs keep their strides
  if (B == 0) return out;
  const int64_t isb = img.stride(0), isc = img.stride(1), isy = img.stride(2), isx = img.stride(3);
  const int64_t osb = out.stride(0), osc = out.stride(1), osy = out.stride(2), osx = out.stride(3);
  TORCH_CHECK(isb >= 0 && isc >= 0 && isy >= 0 && isx >= 0, "color_u8: negative strides");
  const uint8_t* ip = img.data_ptr<uint8_t>();
  uint8_t* op = out.data_ptr<uint8_t>();
  const auto al8 = [](const uint8_t* p, int64_t sb, int64_t sc, int64_t sy, int64_t sx) {
    return sx == 1 && reinterpret_cast<uintptr_t>(p) % 8 == 0 && sb % 8 == 0 && sc % 8 == 0 && sy % 8 == 0;
  };
  const int vec = Ws % 8 == 0 && al8(ip, isb, isc, isy, isx) && al8(op, osb, osc, osy, osx);
  auto sums = torch::empty({B}, plan.options().dtype(torch::kInt32));
  check(pvr_color_u8(ip, isb, isc, isy, isx, op, osb, osc, osy, osx, reinterpret_cast<const pvr::ColorRow*>(plan.data_ptr()),
                     reinterpret_cast<uint32_t*>(sums.data_ptr()), (int)B, (int)Hs, (int)Ws, vec, (int)any_blur, (int)any_sum, stream()),
        "color_u8");
  return out;
}

// xent for soft target rows (mixed label pairs ya / yb with per-row weight lam, label smoothing eps;
// csrc/xent.hip xent_soft_kernel): same outputs as xent, `correct` against ya
torch::Tensor xent_soft(torch::Tensor logits, torch::Tensor ya, torch::Tensor yb, torch::Tensor lam, double eps,
                        c10::optional<torch::Tensor> dlogits, c10::optional<torch::Tensor> correct, double grad_scale,
                        c10::optional<torch::Tensor> mean) {
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1 && logits.size(1) >= 1, "xent_soft: logits must be [B, C] row-major");
  const int64_t B = logits.size(0), C = logits.size(1);
  for (const torch::Tensor* y : {&ya, &yb})
    TORCH_CHECK(y->is_cuda() && y->device() == logits.device() && y->scalar_type() == torch::kInt64 && y->is_contiguous() &&
                    y->numel() == B,
                "xent_soft: ya / yb must be contiguous int64 [B] on the logits' device");
  TORCH_CHECK(lam.device() == logits.device() && lam.is_contiguous() && lam.numel() == B, "xent_soft: lam must be contiguous float32 [B]");
  TORCH_CHECK(eps >= 0.0 && eps <= 1.0, "xent_soft: eps must be in [0, 1], got ", eps);
  if (correct.has_value() && correct->defined())
    TORCH_CHECK(correct->is_cuda() && correct->numel() >= B && correct->scalar_type() == torch::kInt32, "xent_soft: correct int32 [B]");
  if (dlogits.has_value() && dlogits->defined())
    TORCH_CHECK(dlogits->is_cuda() && dlogits->is_contiguous() && dlogits->numel() == B * C && dlogits->scalar_type() == torch::kFloat32,
                "xent_soft: dlogits f32 [B][C]");
  if (mean.has_value() && mean->defined()) TORCH_CHECK(mean->numel() >= 1, "xent_soft: mean [1]");
  auto loss = torch::empty({B}, logits.options().dtype(torch::kFloat32));
  check(pvr_xent_soft(f32(logits, "logits"), logits.stride(0), ya.data_ptr<int64_t>(), yb.data_ptr<int64_t>(), f32(lam, "lam"),
                      (float)eps, (int)B, (int)C, loss.data_ptr<float>(), opt_ptr<float>(dlogits), opt_ptr<int>(correct),
                      (float)grad_scale, stream()),
        "xent_soft");
  if (mean.has_value() && mean->defined()) check(pvr_mean(loss.data_ptr<float>(), (int)B, f32_mut(*mean, "mean"), stream()), "xent_soft mean");
  return loss;
}

// Binary cross-entropy with logits against xent_soft's target rows, binarised at thr when thr >= 0
// (csrc/bce.hip bce_kernel): same outputs as xent_soft. sum_classes: the row loss sums over the classes
// (timm), else it is their mean (BCEWithLogitsLoss); the kernel's row scale follows from it here, so
// that it cannot disagree with C. Everything is checked before the first launch.
torch::Tensor bce(torch::Tensor logits, torch::Tensor ya, torch::Tensor yb, torch::Tensor lam, double eps, double thr,
                  bool sum_classes, c10::optional<torch::Tensor> dlogits, c10::optional<torch::Tensor> correct, double grad_scale,
                  c10::optional<torch::Tensor> mean) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == torch::kFloat32, "bce: logits must be a float32 GPU tensor, got ",
              logits.scalar_type());
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1 && logits.size(1) >= 1, "bce: logits must be [B, C] row-major");
  const int64_t B = logits.size(0), C = logits.size(1);
  // (the kernel's column index advances by 1024 past C in an int)
  TORCH_CHECK(B < (int64_t(1) << 31) && C < (int64_t(1) << 30) && (B <= 1 || logits.stride(0) >= C),
              "bce: logits rows must not overlap, B must fit an int and C be below 2^30");
  for (const torch::Tensor* y : {&ya, &yb})
    TORCH_CHECK(y->is_cuda() && y->device() == logits.device() && y->scalar_type() == torch::kInt64 && y->is_contiguous() &&
                    y->numel() == B,
                "bce: ya / yb must be contiguous int64 [B] on the logits' device");
  TORCH_CHECK(lam.device() == logits.device() && lam.scalar_type() == torch::kFloat32 && lam.is_contiguous() && lam.numel() == B,
              "bce: lam must be contiguous float32 [B] on the logits' device");
  TORCH_CHECK(eps >= 0.0 && eps <= 1.0, "bce: eps must be in [0, 1], got ", eps);
  TORCH_CHECK(thr < 1.0, "bce: thr must be below 1 (negative: no threshold), got ", thr);
  const bool has_dl = dlogits.has_value() && dlogits->defined(), has_corr = correct.has_value() && correct->defined();
  const bool has_mean = mean.has_value() && mean->defined();
  if (has_corr)
    TORCH_CHECK(correct->is_cuda() && correct->device() == logits.device() && correct->is_contiguous() && correct->numel() >= B &&
                    correct->scalar_type() == torch::kInt32,
                "bce: correct int32 [B]");
  if (has_dl)
    TORCH_CHECK(dlogits->is_cuda() && dlogits->device() == logits.device() && dlogits->is_contiguous() && dlogits->numel() == B * C &&
                    dlogits->scalar_type() == torch::kFloat32,
                "bce: dlogits f32 [B][C]");
  if (has_mean)
    TORCH_CHECK(mean->is_cuda() && mean->device() == logits.device() && mean->scalar_type() == torch::kFloat32 && mean->numel() >= 1,
                "bce: mean f32 [1]");
  auto loss = torch::empty({B}, logits.options().dtype(torch::kFloat32));
  const float row_scale = sum_classes ? 1.0f : 1.0f / (float)C;
  check(pvr_bce(logits.data_ptr<float>(), logits.stride(0), ya.data_ptr<int64_t>(), yb.data_ptr<int64_t>(), lam.data_ptr<float>(),
                (float)eps, thr >= 0.0 ? (float)thr : -1.0f, (int)B, (int)C, row_scale, loss.data_ptr<float>(), opt_ptr<float>(dlogits),
                opt_ptr<int>(correct), (float)grad_scale, stream()),
        "bce");
  if (has_mean) check(pvr_mean(loss.data_ptr<float>(), (int)B, mean->data_ptr<float>(), stream()), "bce mean");
  return loss;
}

void cls_rows(torch::Tensor cls, torch::Tensor pos, torch::Tensor out, int64_t B, int64_t D, int64_t row_stride,
              c10::optional<torch::Tensor> seed, int64_t seed_offset, double drop_p) {
  check(pvr_cls_rows(f32(cls, "cls"), f32(pos, "pos"), bf_mut(out, "out"), (int)B, (int)D, row_stride,
                     drop_args(seed, seed_offset, drop_p, "cls_rows"), stream()),
        "cls_rows");
}

void patch_bwd(torch::Tensor dE, int64_t B, int64_t ntok, int64_t D, c10::optional<torch::Tensor> dpos, c10::optional<torch::Tensor> dcls,
               c10::optional<torch::Tensor> dconv, c10::optional<torch::Tensor> dbias, c10::optional<torch::Tensor> seed,
               int64_t seed_offset, double drop_p, c10::optional<torch::Tensor> inv, int64_t n_keep) {
  const pvr::DropSite d = drop_args(seed, seed_offset, drop_p, "patch_bwd");
  const int* ip = nullptr;
  if (inv.has_value() && inv->defined()) {
    // patch dropout: dE / dconv are the compact tensors of n_keep patches per sample, inv the slot table
    TORCH_CHECK(B >= 1 && ntok >= 2 && D >= 8 && D % 8 == 0 && B * ntok < (int64_t(1) << 31), "patch_bwd: sizes");
    TORCH_CHECK(inv->is_cuda() && inv->device() == dE.device() && inv->scalar_type() == torch::kInt32 && inv->is_contiguous() &&
                    inv->dim() == 2 && inv->size(0) == B && inv->size(1) == ntok - 1,
                "patch_bwd: inv must be contiguous int32 [", B, ", ", ntok - 1, "] on dE's device");
    TORCH_CHECK(n_keep >= 1 && n_keep <= ntok - 1, "patch_bwd: n_keep must be in [1, ", ntok - 1, "], got ", n_keep);
    TORCH_CHECK(dE.is_contiguous() && dE.numel() == B * (n_keep + 1) * D, "patch_bwd: dE must be contiguous and hold B * (n_keep + 1) * D elements");
    if (dconv.has_value() && dconv->defined())
      TORCH_CHECK(dconv->is_cuda() && dconv->scalar_type() == torch::kBFloat16 && dconv->is_contiguous() && dconv->numel() == B * n_keep * D,
                  "patch_bwd: dconv must be contiguous bf16 and hold B * n_keep * D elements");
    if (dpos.has_value() && dpos->defined()) TORCH_CHECK(dpos->numel() >= ntok * D, "patch_bwd: dpos must hold ntok * D elements");
    ip = inv->data_ptr<int>();
  } else {
    TORCH_CHECK(dE.numel() == B * ntok * D, "patch_bwd: dE must hold B * ntok * D elements");
  }
  auto ws = torch::empty({pvr_patch_bwd_ws_floats((int)B, (int)ntok, (int)D)}, dE.options().dtype(torch::kFloat32));
  check(pvr_patch_bwd(bf(dE, "dE"), (int)B, (int)ntok, (int)D, ws.data_ptr<float>(), opt_ptr<float>(dpos), opt_ptr<float>(dcls), opt_ptr<uint16_t>(dconv),
                      opt_ptr<float>(dbias), d, ip, (int)n_keep, stream()),
        "patch_bwd");
}

// returns per-row losses; writes dlogits (if given)
// correct (optional): int32 [B], receives 1 where argmax(logits) == label. mean (optional): f32 [1],
// receives the batch mean of the row losses (a second, one-workgroup launch).
torch::Tensor xent(torch::Tensor logits, torch::Tensor labels, c10::optional<torch::Tensor> dlogits, c10::optional<torch::Tensor> correct,
                   double grad_scale, c10::optional<torch::Tensor> mean) {
  TORCH_CHECK(logits.dim() == 2 && logits.stride(1) == 1 && logits.size(1) >= 1, "xent: logits must be [B, C] row-major");
  const int64_t B = logits.size(0), C = logits.size(1);
  // the kernel reads labels[b] for every row b: a short label tensor would be read out of bounds
  TORCH_CHECK(labels.is_cuda() && labels.device() == logits.device() && labels.scalar_type() == torch::kInt64 && labels.is_contiguous() &&
                  labels.numel() == B,
              "xent: labels must be contiguous int64 [B] on the logits' device");
  if (correct.has_value() && correct->defined())
    TORCH_CHECK(correct->is_cuda() && correct->numel() >= B && correct->scalar_type() == torch::kInt32, "xent: correct int32 [B]");
  if (dlogits.has_value() && dlogits->defined())
    TORCH_CHECK(dlogits->is_cuda() && dlogits->is_contiguous() && dlogits->numel() == B * C && dlogits->scalar_type() == torch::kFloat32,
                "xent: dlogits f32 [B][C]");
  if (mean.has_value() && mean->defined()) TORCH_CHECK(mean->numel() >= 1, "xent: mean [1]");
  auto loss = torch::empty({B}, logits.options().dtype(torch::kFloat32));
  check(pvr_xent(f32(logits, "logits"), logits.stride(0), labels.data_ptr<int64_t>(), (int)B, (int)C, loss.data_ptr<float>(),
                 opt_ptr<float>(dlogits), opt_ptr<int>(correct), (float)grad_scale, stream()),
        "xent");
  if (mean.has_value() && mean->defined()) check(pvr_mean(loss.data_ptr<float>(), (int)B, f32_mut(*mean, "mean"), stream()), "xent mean");
  return loss;
}

// The optimizer kernels take raw pointers and element counts: every tensor whose pointer a kernel
// dereferences is checked here, before any launch, for what the kernel assumes of it.
// A flat fp32 buffer read or written as float4: float32, contiguous, 16-byte aligned, on `like`'s device.
void flat_f32(const torch::Tensor& t, const torch::Tensor& like, const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == torch::kFloat32 && t.is_contiguous(), who, ": ", name,
              " must be a contiguous float32 tensor on the GPU of the other buffers");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, who, ": ", name, " must be 16-byte aligned");
}
// A bf16 shadow with the layout of p, written 4 (shadow) or 8 (W^T) values at a time
void flat_bf16(const torch::Tensor& t, const torch::Tensor& like, int64_t align, const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == torch::kBFloat16 && t.is_contiguous(), who, ": ", name,
              " must be a contiguous bfloat16 tensor on the parameters' GPU");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0, who, ": ", name, " must be ", align, "-byte aligned");
}
// {norm, clip coefficient, non-finite flag}: what grad_norm writes and the Adam kernels read
float* clip_triple(const torch::Tensor& t, const torch::Tensor& like, const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.numel() >= 3, who,
              ": ", name, " must be a contiguous float32 tensor of at least 3 elements on the GPU of the other buffers");
  return t.data_ptr<float>();
}
const float* opt_clip(const c10::optional<torch::Tensor>& clip, const torch::Tensor& like, const char* who) {
  return clip.has_value() && clip->defined() ? clip_triple(*clip, like, who, "clip") : nullptr;
}

void grad_norm(torch::Tensor g, double max_norm, torch::Tensor workspace, torch::Tensor out) {
  TORCH_CHECK(g.is_cuda(), "grad_norm: g must be a GPU tensor");
  flat_f32(g, g, "grad_norm", "g");
  TORCH_CHECK(workspace.is_cuda() && workspace.device() == g.device() && workspace.scalar_type() == torch::kFloat32 &&
                  workspace.is_contiguous() && workspace.numel() >= pvr_norm_partial_blocks(),
              "grad_norm: workspace must be a contiguous float32 tensor of at least ", pvr_norm_partial_blocks(), " elements on g's GPU");
  float* po = clip_triple(out, g, "grad_norm", "out");
  check(pvr_grad_norm(g.data_ptr<float>(), g.numel(), (float)max_norm, workspace.data_ptr<float>(), po, stream()), "grad_norm");
}

// Param-group table float32 [G][10] (kernels.h AdamGroup): a CUDA tensor is read by the kernel
// (graph-captured steps); a CPU tensor is copied into the launch's kernel arguments (G <= 8), so an
// eager step needs no host-to-device copy of its per-step lr / bias corrections.
struct GroupTable {
  const pvr::AdamGroup* dev = nullptr;
  const pvr::AdamGroup* host = nullptr;
  int n = 0;
};
GroupTable group_table(const torch::Tensor& groups, const torch::Tensor& p, const char* who) {
  TORCH_CHECK(groups.scalar_type() == torch::kFloat32 && groups.dim() == 2 && groups.size(1) == pvr::ADAM_GROUP_COLS &&
                  groups.is_contiguous(),
              who, ": groups must be contiguous float32 [G, ", pvr::ADAM_GROUP_COLS, "]");
  GroupTable t;
  t.n = (int)groups.size(0);
  auto* ptr = reinterpret_cast<const pvr::AdamGroup*>(groups.data_ptr<float>());
  if (groups.is_cuda()) {
    TORCH_CHECK(groups.device() == p.device() && t.n >= 1, who, ": a device group table holds >= 1 groups on the parameters' GPU");
    t.dev = ptr;
  } else {
    TORCH_CHECK(t.n >= 1 && t.n <= 8, who, ": a host group table holds 1..8 groups (pass a device table for more)");
    t.host = ptr;
  }
  return t;
}

// Model EMA of an Adam pass (kernels.h AdamEma). ema: fp32, contiguous, on p's device, p's numel.
// pair float32 [2] {decay, one_minus_decay}: a CUDA tensor is read by the kernel (graph-captured
// steps), a CPU tensor travels in the kernel arguments. No ema: no EMA (the default kernels).
pvr::AdamEma ema_args(const torch::Tensor& p, c10::optional<torch::Tensor>& ema, const c10::optional<torch::Tensor>& pair, const char* who) {
  pvr::AdamEma a;
  if (!ema.has_value() || !ema->defined()) return a;
  TORCH_CHECK(ema->is_cuda() && ema->device() == p.device() && ema->scalar_type() == torch::kFloat32 && ema->is_contiguous() &&
                  ema->numel() == p.numel(),
              who, ": ema must be contiguous float32 on the parameters' device with their numel");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(ema->data_ptr()) % 16 == 0, who, ": ema must be 16-byte aligned");
  TORCH_CHECK(pair.has_value() && pair->defined() && pair->scalar_type() == torch::kFloat32 && pair->numel() == 2 && pair->is_contiguous(),
              who, ": ema needs ema_pair, float32 [2] {decay, 1 - decay}");
  a.buf = ema->data_ptr<float>();
  if (pair->is_cuda()) {
    TORCH_CHECK(pair->device() == p.device(), who, ": ema_pair on another device");
    a.pair = pair->data_ptr<float>();
  } else {
    a.decay = pair->data_ptr<float>()[0];
    a.one_minus_decay = pair->data_ptr<float>()[1];
  }
  return a;
}

void adam(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v, c10::optional<torch::Tensor> shadow, torch::Tensor seg_start,
          torch::Tensor seg_group, torch::Tensor groups, c10::optional<torch::Tensor> clip, bool skip_nonfinite,
          c10::optional<torch::Tensor> ema, c10::optional<torch::Tensor> ema_pair) {
  TORCH_CHECK(p.is_cuda(), "adam: p must be a GPU tensor");
  flat_f32(p, p, "adam", "p"); flat_f32(g, p, "adam", "g"); flat_f32(m, p, "adam", "m"); flat_f32(v, p, "adam", "v");
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(), "adam: size mismatch");
  TORCH_CHECK(p.numel() % 4 == 0, "adam: the flat buffers hold a multiple of 4 elements (the kernel works in float4), got ", p.numel());
  const GroupTable gt = group_table(groups, p, "adam");
  TORCH_CHECK(seg_start.scalar_type() == torch::kInt64 && seg_group.scalar_type() == torch::kInt32, "adam: segment table dtypes");
  TORCH_CHECK(seg_start.is_cuda() && seg_group.is_cuda() && seg_start.device() == p.device() && seg_group.device() == p.device() &&
                  seg_start.is_contiguous() && seg_group.is_contiguous(),
              "adam: seg_start / seg_group must be contiguous tensors on the parameters' GPU");
  TORCH_CHECK(seg_start.numel() >= 1 && seg_start.numel() == seg_group.numel() && seg_start.numel() < (int64_t(1) << 31),
              "adam: seg_start / seg_group must hold the same number (>= 1) of segments, got ", seg_start.numel(), " and ",
              seg_group.numel());
  uint16_t* sh = nullptr;
  if (shadow.has_value() && shadow->defined()) {
    flat_bf16(*shadow, p, 8, "adam", "shadow");
    TORCH_CHECK(shadow->numel() == p.numel(), "adam: shadow must hold the parameters' ", p.numel(), " elements, got ", shadow->numel());
    sh = reinterpret_cast<uint16_t*>(shadow->data_ptr());
  }
  const float* pc = opt_clip(clip, p, "adam");
  const pvr::AdamEma ea = ema_args(p, ema, ema_pair, "adam");
  check(pvr_adam(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), sh, p.numel(),
                 seg_start.data_ptr<int64_t>(), seg_group.data_ptr<int>(), (int)seg_start.numel(), gt.dev, gt.host, gt.n, pc,
                 skip_nonfinite ? 1 : 0, ea, stream()),
        "adam");
}

// Adam + bf16 shadow + transposed bf16 shadow (W^T of the registered 2-D weights) in one launch.
// tmeta int64 [nmat][6] {flat offset, shadow_t offset, R, C, first tile, group} (R, C % 64 == 0),
// fmeta int64 [nflat][4] {flat start, elements % 4 == 0, group, first float4} for everything else.
void adam_t(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v, torch::Tensor shadow, torch::Tensor shadow_t,
            torch::Tensor tmeta, int64_t ntiles, torch::Tensor fmeta, int64_t flat4, torch::Tensor groups,
            c10::optional<torch::Tensor> clip, bool skip_nonfinite, c10::optional<torch::Tensor> ema,
            c10::optional<torch::Tensor> ema_pair) {
  TORCH_CHECK(p.is_cuda(), "adam_t: p must be a GPU tensor");
  flat_f32(p, p, "adam_t", "p"); flat_f32(g, p, "adam_t", "g"); flat_f32(m, p, "adam_t", "m"); flat_f32(v, p, "adam_t", "v");
  flat_bf16(shadow, p, 8, "adam_t", "shadow");
  flat_bf16(shadow_t, p, 16, "adam_t", "shadow_t");
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel() && shadow.numel() == p.numel(),
              "adam_t: size mismatch");
  const GroupTable gt = group_table(groups, p, "adam_t");
  TORCH_CHECK(tmeta.is_cuda() && tmeta.device() == p.device() && tmeta.scalar_type() == torch::kInt64 && tmeta.dim() == 2 &&
                  tmeta.size(0) >= 1 && tmeta.size(1) == 6 && tmeta.is_contiguous(),
              "adam_t: tmeta int64 [n >= 1][6] on the parameters' GPU");
  TORCH_CHECK(fmeta.is_cuda() && fmeta.device() == p.device() && fmeta.scalar_type() == torch::kInt64 && fmeta.dim() == 2 &&
                  fmeta.size(0) >= 1 && fmeta.size(1) == 4 && fmeta.is_contiguous(),
              "adam_t: fmeta int64 [n >= 1][4] on the parameters' GPU");
  TORCH_CHECK(ntiles >= 1 && ntiles < (int64_t(1) << 31) && flat4 >= 0, "adam_t: ntiles >= 1 and flat4 >= 0");
  const float* pc = opt_clip(clip, p, "adam_t");
  const pvr::AdamEma ea = ema_args(p, ema, ema_pair, "adam_t");
  check(pvr_adam_t(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(),
                   reinterpret_cast<uint16_t*>(shadow.data_ptr()), reinterpret_cast<uint16_t*>(shadow_t.data_ptr()),
                   tmeta.data_ptr<int64_t>(), (int)tmeta.size(0), (int)ntiles, fmeta.data_ptr<int64_t>(), (int)fmeta.size(0), flat4,
                   gt.dev, gt.host, gt.n, pc, skip_nonfinite ? 1 : 0, ea, stream()),
        "adam_t");
}

// LAMB (lamb.hip): three launches over the flat buffers of adam. Segment tables: seg_group int32 [nseg]
// (param group of each parameter tensor, -1 frozen), chunks int64 [nchunks][3] {flat start, elements,
// segment}, seg_chunks int64 [nseg][2] {first chunk, chunks}; partial float32 [nchunks][2], trust
// float32 [nseg][3] {||w||, ||u||, r}.
void lamb_table(const torch::Tensor& t, const torch::Tensor& p, torch::ScalarType dt, int64_t cols, const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == p.device() && t.scalar_type() == dt && t.is_contiguous() && t.numel() < (int64_t(1) << 31) &&
                  (cols == 0 ? t.dim() == 1 : (t.dim() == 2 && t.size(1) == cols)),
              who, ": ", name, " must be a contiguous ", (dt == torch::kInt64 ? "int64" : dt == torch::kInt32 ? "int32" : "float32"),
              cols == 0 ? " vector" : " table", " on the parameters' GPU", cols == 0 ? "" : " with ", cols == 0 ? "" : std::to_string(cols),
              cols == 0 ? "" : " columns");
}

void lamb_moments(torch::Tensor p, torch::Tensor g, torch::Tensor m, torch::Tensor v, torch::Tensor chunks, torch::Tensor seg_group,
                  torch::Tensor partial, torch::Tensor groups, c10::optional<torch::Tensor> clip, bool skip_nonfinite) {
  const char* who = "lamb_moments";
  TORCH_CHECK(p.is_cuda(), who, ": p must be a GPU tensor");
  flat_f32(p, p, who, "p"); flat_f32(g, p, who, "g"); flat_f32(m, p, who, "m"); flat_f32(v, p, who, "v");
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == m.numel() && p.numel() == v.numel(), who, ": size mismatch");
  TORCH_CHECK(p.numel() % 4 == 0, who, ": the flat buffers hold a multiple of 4 elements (the kernel works in float4), got ", p.numel());
  const GroupTable gt = group_table(groups, p, who);
  lamb_table(chunks, p, torch::kInt64, 3, who, "chunks");
  lamb_table(seg_group, p, torch::kInt32, 0, who, "seg_group");
  lamb_table(partial, p, torch::kFloat32, 2, who, "partial");
  TORCH_CHECK(seg_group.numel() >= 1, who, ": seg_group must hold >= 1 segments");
  TORCH_CHECK(partial.size(0) == chunks.size(0), who, ": partial must hold one row per chunk, got ", partial.size(0), " for ", chunks.size(0));
  TORCH_CHECK(reinterpret_cast<uintptr_t>(partial.data_ptr()) % 8 == 0, who, ": partial must be 8-byte aligned");
  const float* pc = opt_clip(clip, p, who);
  check(pvr_lamb_moments(p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), p.numel(),
                         chunks.data_ptr<int64_t>(), (int)chunks.size(0), seg_group.data_ptr<int>(), (int)seg_group.numel(),
                         partial.data_ptr<float>(), gt.dev, gt.host, gt.n, pc, skip_nonfinite ? 1 : 0, stream()),
        who);
}

void lamb_ratio(torch::Tensor partial, torch::Tensor seg_chunks, torch::Tensor seg_group, torch::Tensor trust, torch::Tensor groups,
                c10::optional<torch::Tensor> clip, bool skip_nonfinite) {
  const char* who = "lamb_ratio";
  TORCH_CHECK(trust.is_cuda(), who, ": trust must be a GPU tensor");
  lamb_table(trust, trust, torch::kFloat32, 3, who, "trust");
  lamb_table(partial, trust, torch::kFloat32, 2, who, "partial");
  lamb_table(seg_chunks, trust, torch::kInt64, 2, who, "seg_chunks");
  lamb_table(seg_group, trust, torch::kInt32, 0, who, "seg_group");
  TORCH_CHECK(seg_group.numel() >= 1 && seg_chunks.size(0) == seg_group.numel() && trust.size(0) == seg_group.numel(), who,
              ": seg_chunks, seg_group and trust must hold the same number (>= 1) of segments");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(partial.data_ptr()) % 8 == 0, who, ": partial must be 8-byte aligned");
  const GroupTable gt = group_table(groups, trust, who);
  const float* pc = opt_clip(clip, trust, who);
  check(pvr_lamb_ratio(partial.data_ptr<float>(), (int)partial.size(0), seg_chunks.data_ptr<int64_t>(), seg_group.data_ptr<int>(),
                       (int)seg_group.numel(), trust.data_ptr<float>(), gt.dev, gt.host, gt.n, pc, skip_nonfinite ? 1 : 0, stream()),
        who);
}

// The segment-table form (seg_start, seg_group; shadow optional) or, with shadow_t / tmeta [nmat][7] /
// ntiles / fmeta [nflat][5] / flat4, the tile form that also writes W^T (adam_t's tables with the
// segment index appended to every row).
void lamb_update(torch::Tensor p, torch::Tensor m, torch::Tensor v, c10::optional<torch::Tensor> shadow, torch::Tensor trust,
                 torch::Tensor groups, c10::optional<torch::Tensor> clip, bool skip_nonfinite, c10::optional<torch::Tensor> seg_start,
                 c10::optional<torch::Tensor> seg_group, c10::optional<torch::Tensor> shadow_t, c10::optional<torch::Tensor> tmeta,
                 int64_t ntiles, c10::optional<torch::Tensor> fmeta, int64_t flat4, c10::optional<torch::Tensor> ema,
                 c10::optional<torch::Tensor> ema_pair) {
  const char* who = "lamb_update";
  TORCH_CHECK(p.is_cuda(), who, ": p must be a GPU tensor");
  flat_f32(p, p, who, "p"); flat_f32(m, p, who, "m"); flat_f32(v, p, who, "v");
  TORCH_CHECK(p.numel() == m.numel() && p.numel() == v.numel(), who, ": size mismatch");
  TORCH_CHECK(p.numel() % 4 == 0, who, ": the flat buffers hold a multiple of 4 elements (the kernel works in float4), got ", p.numel());
  const GroupTable gt = group_table(groups, p, who);
  lamb_table(trust, p, torch::kFloat32, 3, who, "trust");
  TORCH_CHECK(trust.size(0) >= 1, who, ": trust must hold >= 1 segments");
  uint16_t* sh = nullptr;
  if (shadow.has_value() && shadow->defined()) {
    flat_bf16(*shadow, p, 8, who, "shadow");
    TORCH_CHECK(shadow->numel() == p.numel(), who, ": shadow must hold the parameters' ", p.numel(), " elements, got ", shadow->numel());
    sh = reinterpret_cast<uint16_t*>(shadow->data_ptr());
  }
  const bool tiles = tmeta.has_value() && tmeta->defined();
  const int64_t* ss = nullptr; const int* sg = nullptr; int nseg = 0;
  uint16_t* sht = nullptr; const int64_t* tm = nullptr; const int64_t* fm = nullptr; int nmat = 0, nflat = 0;
  if (tiles) {
    TORCH_CHECK(sh != nullptr && shadow_t.has_value() && shadow_t->defined() && fmeta.has_value() && fmeta->defined(), who,
                ": the tile form needs shadow, shadow_t, tmeta and fmeta");
    flat_bf16(*shadow_t, p, 16, who, "shadow_t");
    lamb_table(*tmeta, p, torch::kInt64, 7, who, "tmeta");
    lamb_table(*fmeta, p, torch::kInt64, 5, who, "fmeta");
    TORCH_CHECK(tmeta->size(0) >= 1 && fmeta->size(0) >= 1, who, ": tmeta and fmeta hold >= 1 rows");
    TORCH_CHECK(ntiles >= 1 && ntiles < (int64_t(1) << 31) && flat4 >= 0, who, ": ntiles >= 1 and flat4 >= 0");
    sht = reinterpret_cast<uint16_t*>(shadow_t->data_ptr());
    tm = tmeta->data_ptr<int64_t>(); nmat = (int)tmeta->size(0);
    fm = fmeta->data_ptr<int64_t>(); nflat = (int)fmeta->size(0);
  } else {
    TORCH_CHECK(seg_start.has_value() && seg_start->defined() && seg_group.has_value() && seg_group->defined(), who,
                ": the segment-table form needs seg_start and seg_group");
    lamb_table(*seg_start, p, torch::kInt64, 0, who, "seg_start");
    lamb_table(*seg_group, p, torch::kInt32, 0, who, "seg_group");
    TORCH_CHECK(seg_start->numel() >= 1 && seg_start->numel() == seg_group->numel() && trust.size(0) == seg_start->numel(), who,
                ": seg_start, seg_group and trust must hold the same number (>= 1) of segments");
    TORCH_CHECK(ntiles == 0, who, ": ntiles without tmeta");
    ss = seg_start->data_ptr<int64_t>(); sg = seg_group->data_ptr<int>(); nseg = (int)seg_start->numel();
  }
  const float* pc = opt_clip(clip, p, who);
  const pvr::AdamEma ea = ema_args(p, ema, ema_pair, who);
  check(pvr_lamb_update(p.data_ptr<float>(), m.data_ptr<float>(), v.data_ptr<float>(), sh, sht, p.numel(), ss, sg, nseg, tm, nmat,
                        (int)ntiles, fm, nflat, flat4, trust.data_ptr<float>(), gt.dev, gt.host, gt.n, pc, skip_nonfinite ? 1 : 0, ea,
                        stream()),
        who);
}

// SGD (sgd.hip). Its kernels index the flat buffers through the tables, so the tables' contents are checked
// too: once, on the host, when they are built. sgd_segments / sgd_tiles take the tables as CPU tensors,
// check every row against the element counts of the buffers the step will pass, and return an SgdTables
// holding the device copies; sgd / sgd_t take nothing else as tables, so no unchecked row reaches a kernel
// and a step needs no device-to-host copy.
struct SgdTables {
  bool tiles = false;
  torch::Tensor seg_start, seg_group;  // the segment-table form
  torch::Tensor tmeta, fmeta;          // the tile form
  int64_t ntiles = 0, flat4 = 0;
  int64_t n = 0, nt = 0;  // elements of p (g, buf, shadow) and of shadow_t the rows were checked against
  int64_t max_group = -1;  // largest param group a row names
};

void sgd_host_table(const torch::Tensor& t, torch::ScalarType dt, int64_t cols, const char* who, const char* name) {
  TORCH_CHECK(!t.is_cuda() && t.scalar_type() == dt && t.is_contiguous() && t.numel() >= 1 && t.numel() < (int64_t(1) << 31) &&
                  (cols == 0 ? t.dim() == 1 : (t.dim() == 2 && t.size(1) == cols)),
              who, ": ", name, " must be a contiguous ", (dt == torch::kInt64 ? "int64" : "int32"), " CPU ",
              cols == 0 ? "vector" : "table", " of >= 1 rows", cols == 0 ? "" : " with ", cols == 0 ? "" : std::to_string(cols),
              cols == 0 ? "" : " columns");
}

// seg_start int64 [nseg] (sorted, multiples of 4, first 0, inside [0, n)), seg_group int32 [nseg] (-1 frozen)
SgdTables sgd_segments(torch::Tensor seg_start, torch::Tensor seg_group, int64_t n, torch::Device device) {
  const char* who = "sgd_segments";
  sgd_host_table(seg_start, torch::kInt64, 0, who, "seg_start");
  sgd_host_table(seg_group, torch::kInt32, 0, who, "seg_group");
  TORCH_CHECK(seg_start.numel() == seg_group.numel(), who, ": seg_start / seg_group must hold the same number of segments, got ",
              seg_start.numel(), " and ", seg_group.numel());
  TORCH_CHECK(n >= 4 && n % 4 == 0, who, ": the flat buffers hold a multiple of 4 elements (the kernel works in float4), got ", n);
  TORCH_CHECK(device.is_cuda(), who, ": device must be a GPU");
  SgdTables t;
  const int64_t* ss = seg_start.data_ptr<int64_t>();
  const int* sg = seg_group.data_ptr<int>();
  for (int64_t i = 0; i < seg_start.numel(); ++i) {
    TORCH_CHECK(ss[i] % 4 == 0, who, ": segment ", i, " starts at element ", ss[i], ", not a multiple of 4 (the kernel works in float4)");
    TORCH_CHECK(i == 0 ? ss[i] == 0 : ss[i] > ss[i - 1], who, ": seg_start must begin at 0 and rise strictly (segment ", i, ")");
    TORCH_CHECK(ss[i] < n, who, ": segment ", i, " starts at element ", ss[i], " of ", n);
    TORCH_CHECK(sg[i] >= -1, who, ": segment ", i, " names group ", sg[i]);
    t.max_group = std::max<int64_t>(t.max_group, sg[i]);
  }
  t.n = n;
  t.seg_start = seg_start.to(device);
  t.seg_group = seg_group.to(device);
  return t;
}

// tmeta int64 [nmat][6] {flat offset, shadow_t offset, R, C, first tile, group} (R, C % 64 == 0),
// fmeta int64 [nflat][4] {flat start, elements % 4 == 0, group, first float4}: adam_t's tables.
// n / nt: elements of the flat buffers and of shadow_t.
SgdTables sgd_tiles(torch::Tensor tmeta, torch::Tensor fmeta, int64_t n, int64_t nt, torch::Device device) {
  const char* who = "sgd_tiles";
  sgd_host_table(tmeta, torch::kInt64, 6, who, "tmeta");
  sgd_host_table(fmeta, torch::kInt64, 4, who, "fmeta");
  TORCH_CHECK(n >= 4 && n % 4 == 0 && nt >= 0, who, ": the flat buffers hold a multiple of 4 elements, got ", n);
  TORCH_CHECK(device.is_cuda(), who, ": device must be a GPU");
  SgdTables t;
  t.tiles = true;
  const int64_t* tm = tmeta.data_ptr<int64_t>();
  for (int64_t i = 0; i < tmeta.size(0); ++i, tm += 6) {
    const int64_t soff = tm[0], doff = tm[1], R = tm[2], C = tm[3];
    TORCH_CHECK(R >= 64 && C >= 64 && R % 64 == 0 && C % 64 == 0 && R < (int64_t(1) << 24) && C < (int64_t(1) << 24), who, ": matrix ",
                i, " is ", R, " x ", C, ", not multiples of 64");
    TORCH_CHECK(soff >= 0 && soff % 4 == 0 && soff + R * C <= n, who, ": matrix ", i, " at element ", soff,
                " must start at a multiple of 4 and lie inside the ", n, " elements of the buffers");
    TORCH_CHECK(doff >= 0 && doff % 8 == 0 && doff + R * C <= nt, who, ": W^T of matrix ", i, " at element ", doff,
                " must start at a multiple of 8 and lie inside the ", nt, " elements of shadow_t");
    TORCH_CHECK(tm[4] == t.ntiles, who, ": matrix ", i, " must name its first tile, ", t.ntiles, ", got ", tm[4]);
    TORCH_CHECK(tm[5] >= -1 && tm[5] < (int64_t(1) << 31), who, ": matrix ", i, " names group ", tm[5]);
    t.ntiles += (R / 64) * (C / 64);
    t.max_group = std::max(t.max_group, tm[5]);
  }
  TORCH_CHECK(t.ntiles < (int64_t(1) << 31), who, ": too many tiles");
  const int64_t* fm = fmeta.data_ptr<int64_t>();
  for (int64_t i = 0; i < fmeta.size(0); ++i, fm += 4) {
    TORCH_CHECK(fm[0] >= 0 && fm[0] % 4 == 0 && fm[1] >= 4 && fm[1] % 4 == 0 && fm[1] <= n && fm[0] <= n - fm[1], who, ": range ", i,
                " (start ", fm[0], ", ", fm[1], " elements) must start at and hold a multiple of 4 inside the ", n,
                " elements of the buffers");
    TORCH_CHECK(fm[3] == t.flat4, who, ": range ", i, " must name its first float4, ", t.flat4, ", got ", fm[3]);
    TORCH_CHECK(fm[2] >= -1 && fm[2] < (int64_t(1) << 31), who, ": range ", i, " names group ", fm[2]);
    t.flat4 += fm[1] / 4;
    t.max_group = std::max(t.max_group, fm[2]);
  }
  t.n = n;
  t.nt = nt;
  t.tmeta = tmeta.to(device);
  t.fmeta = fmeta.to(device);
  return t;
}

// What sgd and sgd_t share: the buffers against the element count the tables were checked for
const GroupTable sgd_common(const SgdTables& t, const torch::Tensor& p, const torch::Tensor& g, const torch::Tensor& buf,
                            const torch::Tensor& groups, const char* who) {
  TORCH_CHECK(p.is_cuda(), who, ": p must be a GPU tensor");
  flat_f32(p, p, who, "p"); flat_f32(g, p, who, "g"); flat_f32(buf, p, who, "buf");
  TORCH_CHECK(p.numel() == g.numel() && p.numel() == buf.numel(), who, ": size mismatch");
  TORCH_CHECK(p.numel() == t.n, who, ": the tables were built for buffers of ", t.n, " elements, got ", p.numel());
  const GroupTable gt = group_table(groups, p, who);
  TORCH_CHECK(t.max_group < gt.n, who, ": the tables name group ", t.max_group, ", the group table holds ", gt.n);
  return gt;
}

void sgd(torch::Tensor p, torch::Tensor g, torch::Tensor buf, c10::optional<torch::Tensor> shadow, const SgdTables& tables,
         torch::Tensor groups, c10::optional<torch::Tensor> clip, bool skip_nonfinite, c10::optional<torch::Tensor> ema,
         c10::optional<torch::Tensor> ema_pair) {
  const char* who = "sgd";
  TORCH_CHECK(!tables.tiles, who, ": tables of the tile form (sgd_tiles) go to sgd_t");
  const GroupTable gt = sgd_common(tables, p, g, buf, groups, who);
  TORCH_CHECK(tables.seg_start.device() == p.device(), who, ": the tables are on another device");
  uint16_t* sh = nullptr;
  if (shadow.has_value() && shadow->defined()) {
    flat_bf16(*shadow, p, 8, who, "shadow");
    TORCH_CHECK(shadow->numel() == p.numel(), who, ": shadow must hold the parameters' ", p.numel(), " elements, got ", shadow->numel());
    sh = reinterpret_cast<uint16_t*>(shadow->data_ptr());
  }
  const float* pc = opt_clip(clip, p, who);
  const pvr::AdamEma ea = ema_args(p, ema, ema_pair, who);
  check(pvr_sgd(p.data_ptr<float>(), g.data_ptr<float>(), buf.data_ptr<float>(), sh, p.numel(), tables.seg_start.data_ptr<int64_t>(),
                tables.seg_group.data_ptr<int>(), (int)tables.seg_start.numel(), gt.dev, gt.host, gt.n, pc, skip_nonfinite ? 1 : 0, ea,
                stream()),
        who);
}

void sgd_t(torch::Tensor p, torch::Tensor g, torch::Tensor buf, torch::Tensor shadow, torch::Tensor shadow_t, const SgdTables& tables,
           torch::Tensor groups, c10::optional<torch::Tensor> clip, bool skip_nonfinite, c10::optional<torch::Tensor> ema,
           c10::optional<torch::Tensor> ema_pair) {
  const char* who = "sgd_t";
  TORCH_CHECK(tables.tiles, who, ": tables of the segment form (sgd_segments) go to sgd");
  const GroupTable gt = sgd_common(tables, p, g, buf, groups, who);
  TORCH_CHECK(tables.tmeta.device() == p.device(), who, ": the tables are on another device");
  flat_bf16(shadow, p, 8, who, "shadow");
  flat_bf16(shadow_t, p, 16, who, "shadow_t");
  TORCH_CHECK(shadow.numel() == p.numel(), who, ": shadow must hold the parameters' ", p.numel(), " elements, got ", shadow.numel());
  TORCH_CHECK(shadow_t.numel() == tables.nt, who, ": the tables were built for a shadow_t of ", tables.nt, " elements, got ",
              shadow_t.numel());
  const float* pc = opt_clip(clip, p, who);
  const pvr::AdamEma ea = ema_args(p, ema, ema_pair, who);
  check(pvr_sgd_t(p.data_ptr<float>(), g.data_ptr<float>(), buf.data_ptr<float>(), reinterpret_cast<uint16_t*>(shadow.data_ptr()),
                  reinterpret_cast<uint16_t*>(shadow_t.data_ptr()), tables.tmeta.data_ptr<int64_t>(), (int)tables.tmeta.size(0),
                  (int)tables.ntiles, tables.fmeta.data_ptr<int64_t>(), (int)tables.fmeta.size(0), tables.flat4, gt.dev, gt.host, gt.n,
                  pc, skip_nonfinite ? 1 : 0, ea, stream()),
        who);
}

// Classifier head forward: LayerNorm of each image's CLS row (token 0 of tokens [B*N][D] bf16) and
// logits = LN(x) . W^T + bias in fp32. Returns {logits [B][C], xhat [B][D], rstd [B]} (the latter two
// saved for head_bwd).
std::vector<torch::Tensor> head_fwd(torch::Tensor tokens, int64_t B, int64_t N, torch::Tensor gamma, torch::Tensor beta, double eps,
                                    torch::Tensor W, c10::optional<torch::Tensor> bias) {
  const int64_t D = tokens.size(1);
  TORCH_CHECK(tokens.dim() == 2 && tokens.size(0) == B * N && tokens.is_contiguous(), "head_fwd: tokens [B*N][D] contiguous");
  TORCH_CHECK(D % 16 == 0 && D <= 1536, "head_fwd: D % 16 == 0, D <= 1536");
  TORCH_CHECK(W.dim() == 2 && W.size(1) == D && W.is_contiguous() && gamma.numel() == D && beta.numel() == D, "head_fwd: shapes");
  const int64_t C = W.size(0);
  const float* bp = nullptr;
  if (bias.has_value() && bias->defined()) { TORCH_CHECK(bias->numel() == C && bias->is_contiguous(), "head_fwd: bias [C]"); bp = f32(*bias, "bias"); }
  auto f = tokens.options().dtype(torch::kFloat32);
  auto logits = torch::empty({B, C}, f);
  auto xhat = torch::empty({B, D}, f);
  auto rstd = torch::empty({B}, f);
  check(pvr_head_fwd(bf(tokens, "tokens"), N * D, (int)B, (int)D, f32(gamma, "gamma"), f32(beta, "beta"), (float)eps, f32(W, "W"), bp,
                     (int)C, xhat.data_ptr<float>(), rstd.data_ptr<float>(), logits.data_ptr<float>(), stream()),
        "head_fwd");
  return {logits, xhat, rstd};
}

// Classifier head backward: dW / db / dgamma / dbeta accumulate (+=) into the given fp32 gradients
// (each optional), returns d(tokens) [B*N][D] bf16: the LayerNorm backward in every CLS row, zeros
// elsewhere (written by the same launch).
torch::Tensor head_bwd(torch::Tensor dlogits, torch::Tensor xhat, torch::Tensor rstd, torch::Tensor gamma, torch::Tensor beta,
                       torch::Tensor W, int64_t B, int64_t N, c10::optional<torch::Tensor> dW, c10::optional<torch::Tensor> db,
                       c10::optional<torch::Tensor> dgamma, c10::optional<torch::Tensor> dbeta) {
  const int64_t C = W.size(0), D = W.size(1);
  TORCH_CHECK(dlogits.dim() == 2 && dlogits.size(0) == B && dlogits.size(1) == C && dlogits.is_contiguous(), "head_bwd: dlogits [B][C]");
  TORCH_CHECK(xhat.numel() == B * D && rstd.numel() == B && W.is_contiguous(), "head_bwd: saved tensors");
  float* pdw = opt_ptr<float>(dW);
  if (pdw) TORCH_CHECK(dW->numel() == C * D && dW->is_contiguous() && dW->scalar_type() == torch::kFloat32, "head_bwd: dW");
  auto dy = torch::empty({B, D}, xhat.options());
  auto dtok = torch::empty({B * N, D}, xhat.options().dtype(torch::kBFloat16));
  check(pvr_head_bwd(f32(dlogits, "dlogits"), f32(xhat, "xhat"), f32(rstd, "rstd"), f32(gamma, "gamma"), f32(beta, "beta"), f32(W, "W"),
                     (int)B, (int)C, (int)D, (int)N, pdw, opt_ptr<float>(db), opt_ptr<float>(dgamma), opt_ptr<float>(dbeta),
                     dy.data_ptr<float>(), reinterpret_cast<uint16_t*>(dtok.data_ptr()),
                     g_deterministic && (opt_ptr<float>(dgamma) || opt_ptr<float>(dbeta)) ? det_scratch(((B + 15) / 16) * 2 * D, xhat.options()) : nullptr, stream()),
        "head_bwd");
  return dtok;
}

// y = x * s[0] (s a 1-element device tensor): the cross-entropy backward's upstream-gradient scale
torch::Tensor scale_by(torch::Tensor x, torch::Tensor s) {
  TORCH_CHECK(x.is_contiguous() && s.numel() >= 1, "scale_by: contiguous x, scalar s");
  auto y = torch::empty_like(x);
  check(pvr_scale_by(f32(x, "x"), f32(s, "s"), y.data_ptr<float>(), x.numel(), stream()), "scale_by");
  return y;
}

// sums[0] += loss[0]; sums[1] += sum(correct) / B with correct = xent's per-row flags [B] (per-batch
// metrics accumulated on the device)
void metrics_accum(torch::Tensor sums, torch::Tensor loss, torch::Tensor correct) {
  TORCH_CHECK(sums.numel() >= 2 && correct.scalar_type() == torch::kInt32 && correct.is_contiguous(),
              "metrics_accum: sums [2] f32, correct int32 [B]");
  check(pvr_metrics_accum(f32_mut(sums, "sums"), f32(loss, "loss"), correct.data_ptr<int>(), (int)correct.numel(), stream()),
        "metrics_accum");
}

void rng_next(torch::Tensor rng, torch::Tensor seed) {
  TORCH_CHECK(rng.is_cuda() && seed.is_cuda() && rng.scalar_type() == torch::kInt64 && seed.scalar_type() == torch::kInt64 &&
                  rng.numel() >= 1 && seed.numel() >= 1,
              "rng_next: int64 device tensors");
  check(pvr_rng_next(rng.data_ptr<int64_t>(), seed.data_ptr<int64_t>(), stream()), "rng_next");
}

void zero_f32(torch::Tensor x) {
  TORCH_CHECK(x.is_contiguous() && x.numel() % 4 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0,
              "zero_f32: contiguous, 16-B aligned, numel % 4 == 0");
  check(pvr_zero_f32(f32_mut(x, "x"), x.numel(), stream()), "zero_f32");
}

// LayerScale fold (csrc/layerscale.hip): meta int64 [n][8] on the GPU with meta_host, the same rows on the
// host, which are what is validated here: every matrix, scale and bias inside `master`, every output
// inside w16 / wt16 / bhat, R, C and the offsets multiples of 8, the tile prefixes those of the rows.
void layerscale_fold(torch::Tensor master, torch::Tensor w16, torch::Tensor wt16, torch::Tensor bhat, torch::Tensor meta,
                     torch::Tensor meta_host) {
  TORCH_CHECK(master.dim() == 1 && w16.dim() == 1 && wt16.dim() == 1 && bhat.dim() == 1 && master.is_contiguous() &&
                  w16.is_contiguous() && wt16.is_contiguous() && bhat.is_contiguous(),
              "layerscale_fold: master, w16, wt16 and bhat must be flat contiguous buffers");
  const float* mp = f32(master, "master");
  uint16_t* wp = bf_mut(w16, "w16");
  uint16_t* wtp = bf_mut(wt16, "wt16");
  float* bp = f32_mut(bhat, "bhat");
  TORCH_CHECK(w16.device() == master.device() && wt16.device() == master.device() && bhat.device() == master.device() &&
                  meta.is_cuda() && meta.device() == master.device(),
              "layerscale_fold: every buffer and meta on the same GPU");
  TORCH_CHECK(w16.numel() == wt16.numel() && w16.data_ptr() != wt16.data_ptr(), "layerscale_fold: w16 and wt16 are two buffers of one size");
  for (const void* p : {(const void*)mp, (const void*)wp, (const void*)wtp, (const void*)bp})
    TORCH_CHECK(reinterpret_cast<uintptr_t>(p) % 16 == 0, "layerscale_fold: buffers must be 16-byte aligned");
  TORCH_CHECK(meta.scalar_type() == torch::kInt64 && meta.dim() == 2 && meta.size(1) == 8 && meta.is_contiguous(),
              "layerscale_fold: meta must be int64 [n, 8]");
  TORCH_CHECK(!meta_host.is_cuda() && meta_host.scalar_type() == torch::kInt64 && meta_host.is_contiguous() &&
                  meta_host.sizes() == meta.sizes(),
              "layerscale_fold: meta_host must be the host copy of meta (int64 [n, 8])");
  const int64_t n = meta.size(0);
  const int64_t* h = meta_host.data_ptr<int64_t>();
  int64_t tiles = 0;
  for (int64_t t = 0; t < n; ++t) {
    const int64_t woff = h[t * 8], goff = h[t * 8 + 1], boff = h[t * 8 + 2], R = h[t * 8 + 3], C = h[t * 8 + 4];
    const int64_t ooff = h[t * 8 + 5], hoff = h[t * 8 + 6];
    TORCH_CHECK(R > 0 && C > 0 && R % 8 == 0 && C % 8 == 0 && R < (1 << 24) && C < (1 << 24),
                "layerscale_fold: R and C must be positive multiples of 8, got ", R, " x ", C);
    TORCH_CHECK(woff >= 0 && goff >= 0 && boff >= 0 && ooff >= 0 && hoff >= 0 && woff % 8 == 0 && ooff % 8 == 0,
                "layerscale_fold: offsets must be non-negative, those of W and of its copies multiples of 8");
    TORCH_CHECK(woff + R * C <= master.numel() && goff + R <= master.numel() && boff + R <= master.numel(),
                "layerscale_fold: row ", t, " reads outside master");
    TORCH_CHECK(ooff + R * C <= w16.numel() && hoff + R <= bhat.numel(), "layerscale_fold: row ", t, " writes outside its output");
    TORCH_CHECK(h[t * 8 + 7] == tiles, "layerscale_fold: row ", t, " tile prefix");
    tiles += ((R + 63) / 64) * ((C + 63) / 64);
  }
  TORCH_CHECK(tiles < (int64_t(1) << 31), "layerscale_fold: too many tiles");
  check(pvr_layerscale_fold(mp, wp, wtp, bp, meta.data_ptr<int64_t>(), (int)n, (int)tiles, stream()), "layerscale_fold");
}

// LayerScale unfold (csrc/layerscale.hip): gW / gb / gg (each optional) += the gradients of W [R, C], b [R]
// and the scale g [R] from dw_hat [R, C] and db_hat [R], the gradients of the folded pair.
void layerscale_unfold(torch::Tensor dw_hat, torch::Tensor db_hat, torch::Tensor W, torch::Tensor b, torch::Tensor g,
                       c10::optional<torch::Tensor> gW, c10::optional<torch::Tensor> gb, c10::optional<torch::Tensor> gg) {
  TORCH_CHECK(W.dim() == 2 && W.is_contiguous(), "layerscale_unfold: W must be a contiguous [R, C] matrix");
  const int64_t R = W.size(0), C = W.size(1);
  TORCH_CHECK(R > 0 && C > 0 && R % 8 == 0 && C % 8 == 0 && R < (int64_t(1) << 31) && C < (int64_t(1) << 31),
              "layerscale_unfold: R and C must be positive multiples of 8, got ", R, " x ", C);
  bool vec = true;
  auto mat = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.dim() == 2 && t.size(0) == R && t.size(1) == C && t.is_contiguous() && t.device() == W.device(),
                "layerscale_unfold: ", name, " must be a contiguous [", R, ", ", C, "] matrix on W's GPU");
    vec = vec && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
    return f32(t, name);
  };
  auto vecr = [&](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.dim() == 1 && t.size(0) == R && t.is_contiguous() && t.device() == W.device(),
                "layerscale_unfold: ", name, " must be a contiguous [", R, "] vector on W's GPU");
    return f32(t, name);
  };
  const float* wp = mat(W, "W");
  const float* dwp = mat(dw_hat, "dw_hat");
  const float* dbp = vecr(db_hat, "db_hat");
  const float* bp = vecr(b, "b");
  const float* gp = vecr(g, "g");
  float* gWp = gW.has_value() && gW->defined() ? const_cast<float*>(mat(*gW, "gW")) : nullptr;
  float* gbp = gb.has_value() && gb->defined() ? const_cast<float*>(vecr(*gb, "gb")) : nullptr;
  float* ggp = gg.has_value() && gg->defined() ? const_cast<float*>(vecr(*gg, "gg")) : nullptr;
  check(pvr_layerscale_unfold(dwp, dbp, wp, bp, gp, gWp, gbp, ggp, (int)R, (int)C, vec ? 1 : 0, stream()), "layerscale_unfold");
}

void scale_by_clip(torch::Tensor g, torch::Tensor clip) {
  check(pvr_scale_by_clip(f32_mut(g, "g"), g.numel(), f32(clip, "clip"), stream()), "scale_by_clip");
}

const uint8_t* u8(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kUInt8, name, " must hold fp8 bytes (uint8), got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.stride(1) == 1 && t.stride(0) % 16 == 0, name, " must be 2-D with a 16-byte multiple row stride");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name, " must be 16-byte aligned");
  return reinterpret_cast<const uint8_t*>(t.data_ptr());
}

// C[M][N] = epilogue(dscale_a * dscale_b * A[M][K] . B[N][K]^T), A/B OCP fp8 (fmt 0 e4m3, 1 e5m2)
void gemm_fp8(torch::Tensor A, int64_t fmt_a, torch::Tensor B, int64_t fmt_b, torch::Tensor C, int64_t M, int64_t N, int64_t K,
              int64_t epi, torch::Tensor scale_a, torch::Tensor scale_b, c10::optional<torch::Tensor> bias,
              c10::optional<torch::Tensor> resid, c10::optional<torch::Tensor> aux, c10::optional<torch::Tensor> seed, int64_t seed_offset,
              double drop_p, c10::optional<torch::Tensor> colsum, c10::optional<torch::Tensor> q_out,
              c10::optional<torch::Tensor> q_scale, c10::optional<torch::Tensor> q_amax, int64_t q_fmt, bool c_skip,
              int64_t tail_limit) {
  pvr::GemmParams p{};
  // c_skip: only the fp8 copy (or aux / column sums) of the output is consumed; the bf16 stores are
  // dropped (register-direct epilogue; other epilogues still write C, which is allocated)
  TORCH_CHECK(!c_skip || epi == 1 || epi == 2, "gemm_fp8: c_skip with the GELU / dGELU epilogues only");
  p.c_skip = c_skip ? 1 : 0;
  p.drop_scale = 1.f;
  p.M = (int)M; p.N = (int)N; p.K = (int)K;
  p.A = reinterpret_cast<const uint16_t*>(u8(A, "A")); p.lda = A.stride(0); p.a_kcontig = 1;
  p.B = reinterpret_cast<const uint16_t*>(u8(B, "B")); p.ldb = B.stride(0); p.b_kcontig = 1;
  TORCH_CHECK(A.size(0) >= M && A.size(1) >= K && B.size(0) >= N && B.size(1) >= K, "gemm_fp8: operand too small");
  TORCH_CHECK(K % 128 == 0 && N % 8 == 0, "gemm_fp8: K must be a multiple of 128, N of 8");
  TORCH_CHECK(C.is_cuda() && C.scalar_type() == torch::kBFloat16, "gemm_fp8: bf16 output");
  p.C = C.data_ptr(); p.ldc = ld_of(C, "C");
  p.scale_a = f32(scale_a, "scale_a"); p.scale_b = f32(scale_b, "scale_b");
  p.elem8 = 1; p.fmt_a = (int)fmt_a; p.fmt_b = (int)fmt_b;
  if (bias.has_value() && bias->defined()) { TORCH_CHECK(bias->numel() >= N && bias->is_contiguous(), "bias"); p.bias = f32(*bias, "bias"); }
  if (resid.has_value() && resid->defined()) { p.resid = bf(*resid, "resid"); p.ld_resid = ld_of(*resid, "resid"); }
  if (aux.has_value() && aux->defined()) { p.aux = const_cast<uint16_t*>(bf(*aux, "aux")); p.ld_aux = ld_of(*aux, "aux"); }
  // GELU without aux: the inference epilogue (no derivative stored; its stores go to a 0-byte range)
  if (epi == 2) TORCH_CHECK(p.aux != nullptr, "gemm_fp8: the dGELU epilogue needs aux");
  if (colsum.has_value() && colsum->defined()) p.colsum = f32_mut(*colsum, "colsum");
  if (q_out.has_value() && q_out->defined()) {
    // fp8 copy of the GELU / dGELU output from the register-direct epilogue (its preconditions:
    // 16-B column groups, 31-bit offsets of every row-major operand it touches)
    TORCH_CHECK(epi == 1 || epi == 2, "gemm_fp8: q_out with the GELU / dGELU epilogues only");
    const pvr::Fp8Copy q = fp8_copy(q_out, q_scale, q_amax, q_fmt, M, N, 8, "gemm_fp8");
    const int64_t ld_max = std::max(std::max(p.ldc, p.ld_aux), std::max(p.ld_resid, (int64_t)N));
    TORCH_CHECK(M * ld_max * 2 < (1ll << 31), "gemm_fp8: q_out path needs 31-bit output offsets");
    p.q_out = q.out; p.ld_q = q.ld; p.q_scale = q.scale; p.q_amax = q.amax; p.q_fmt = q.fmt;
  }
  set_drop(p, drop_args(seed, seed_offset, drop_p, "gemm_fp8"));
  p.k_split_len = (int)K;
  p.epi = (int)epi;
  p.tile_cfg = 12;
  if (epi <= 2 && tail_limit >= 0) {  // tail_limit: as for gemm()
    attach_tail(p, C);
    p.tail_max_units = (int)tail_limit;
    p.tail_min_kt = g_tail_min_kt;
  }
  check(pvr_gemm(&p, stream()), "gemm_fp8");
}

// yT[cols][ldy] (uint8 fp8) = sat(x^T * qscale), zero past x's rows (ldy: token dim padded to 128)
void fp8_quant_t(torch::Tensor x, torch::Tensor yt, torch::Tensor qscale, int64_t fmt) {
  TORCH_CHECK(x.dim() == 2 && yt.dim() == 2 && yt.size(0) == x.size(1) && yt.size(1) >= x.size(0) && yt.stride(1) == 1,
              "fp8_quant_t: yT [cols][>= rows]");
  TORCH_CHECK(yt.is_cuda() && yt.scalar_type() == torch::kUInt8 && yt.stride(0) % 64 == 0 && yt.size(1) == yt.stride(0),
              "fp8_quant_t: yT uint8, row stride a multiple of 64");
  check(pvr_fp8_quant_t(bf(x, "x"), ld_of(x, "x"), yt.data_ptr<uint8_t>(), yt.stride(0), (int)x.size(0), (int)x.size(1),
                        f32(qscale, "qscale"), (int)fmt, stream()),
        "fp8_quant_t");
}

// yT[cols][ldy] = x8^T (fp8 bytes), zero past x8's rows: the transposed wgrad operand from a row-major fp8 copy
void fp8_transpose(torch::Tensor x8, torch::Tensor yt) {
  TORCH_CHECK(x8.is_cuda() && x8.scalar_type() == torch::kUInt8 && x8.dim() == 2 && x8.stride(1) == 1 && x8.stride(0) % 16 == 0 &&
                  x8.size(1) % 16 == 0 && reinterpret_cast<uintptr_t>(x8.data_ptr()) % 16 == 0,
              "fp8_transpose: x8 uint8 [rows][cols], cols and row stride multiples of 16, 16-byte aligned");
  TORCH_CHECK(yt.is_cuda() && yt.scalar_type() == torch::kUInt8 && yt.dim() == 2 && yt.size(0) == x8.size(1) &&
                  yt.size(1) >= x8.size(0) && yt.stride(1) == 1 && yt.stride(0) % 64 == 0 && yt.size(1) == yt.stride(0) &&
                  reinterpret_cast<uintptr_t>(yt.data_ptr()) % 16 == 0,
              "fp8_transpose: yT uint8 [cols][>= rows], row stride a multiple of 64");
  check(pvr_fp8_transpose(x8.data_ptr<uint8_t>(), x8.stride(0), yt.data_ptr<uint8_t>(), yt.stride(0), (int)x8.size(0), (int)x8.size(1),
                          stream()),
        "fp8_transpose");
}

// fp8 weight gradient partials straight from the row-major fp8 copies: ws[s][N][K] = dscale_a *
// dscale_b * dy8[Ts][N]^T . x8[Ts][K] over token split s (ksplit tokens, a multiple of 128), dy8 e5m2
// (fmt_a 1) or e4m3 (fmt_a 0)
// and x8 e4m3 [T][features] (mn-contiguous operands: transposed LDS reads, no transposed copies)
void gemm_fp8_wgrad_mn(torch::Tensor dy8, torch::Tensor x8, torch::Tensor ws, int64_t N, int64_t K, int64_t T, torch::Tensor scale_a,
                       torch::Tensor scale_b, int64_t ksplit, int64_t fmt_a) {
  TORCH_CHECK((fmt_a == 0 || fmt_a == 1), "gemm_fp8_wgrad_mn: fmt_a 0 (e4m3) / 1 (e5m2)");
  TORCH_CHECK(dy8.dim() == 2 && x8.dim() == 2 && dy8.size(0) >= T && x8.size(0) >= T && dy8.size(1) >= N && x8.size(1) >= K &&
                  dy8.stride(1) == 1 && x8.stride(1) == 1,
              "gemm_fp8_wgrad_mn: dy8 [T][N], x8 [T][K] row-major");
  TORCH_CHECK(N % 16 == 0 && K % 16 == 0 && dy8.stride(0) % 16 == 0 && x8.stride(0) % 16 == 0 && ksplit % 128 == 0 &&
                  reinterpret_cast<uintptr_t>(dy8.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(x8.data_ptr()) % 16 == 0,
              "gemm_fp8_wgrad_mn: 16-byte rows and bases, ksplit a multiple of 128");
  TORCH_CHECK(T * std::max(dy8.stride(0), x8.stride(0)) < (1ll << 31), "gemm_fp8_wgrad_mn: 31-bit operand offsets");
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == torch::kFloat32 && ws.dim() == 3 && ws.stride(2) == 1 && ws.size(1) >= N &&
                  ws.size(2) >= K && ws.size(0) >= (T + ksplit - 1) / ksplit,
              "gemm_fp8_wgrad_mn: workspace [splits][N][K] f32");
  pvr::GemmParams p{};
  p.drop_scale = 1.f;
  p.M = (int)N; p.N = (int)K; p.K = (int)T;
  p.A = reinterpret_cast<const uint16_t*>(u8(dy8, "dy8")); p.lda = dy8.stride(0); p.a_kcontig = 0;
  p.B = reinterpret_cast<const uint16_t*>(u8(x8, "x8")); p.ldb = x8.stride(0); p.b_kcontig = 0;
  p.C = ws.data_ptr(); p.ldc = ws.stride(1); p.split_stride = ws.stride(0);
  p.scale_a = f32(scale_a, "scale_a"); p.scale_b = f32(scale_b, "scale_b");
  p.elem8 = 1; p.fmt_a = (int)fmt_a; p.fmt_b = 0;
  p.k_split_len = (int)ksplit;
  p.epi = 4;  // EPI_F32_STORE
  p.tile_cfg = 14;
  check(pvr_gemm(&p, stream()), "gemm_fp8_wgrad_mn");
}

// fp8 weight gradient partials: ws[s][N][K] = dscale_a * dscale_b * A8[N][Ks] . B8[K][Ks]^T over split s
// of the (padded) token dim, A e5m2 / e4m3 (fmt_a 1 / 0; gradient^T), B e4m3 (activation^T)
void gemm_fp8_wgrad(torch::Tensor A8, torch::Tensor B8, torch::Tensor ws, int64_t N, int64_t K, int64_t Tp, torch::Tensor scale_a,
                    torch::Tensor scale_b, int64_t ksplit, int64_t fmt_a) {
  TORCH_CHECK((fmt_a == 0 || fmt_a == 1), "gemm_fp8_wgrad: fmt_a 0 (e4m3) / 1 (e5m2)");
  pvr::GemmParams p{};
  p.drop_scale = 1.f;
  p.M = (int)N; p.N = (int)K; p.K = (int)Tp;
  p.A = reinterpret_cast<const uint16_t*>(u8(A8, "A8")); p.lda = A8.stride(0); p.a_kcontig = 1;
  p.B = reinterpret_cast<const uint16_t*>(u8(B8, "B8")); p.ldb = B8.stride(0); p.b_kcontig = 1;
  TORCH_CHECK(A8.size(0) >= N && A8.size(1) >= Tp && B8.size(0) >= K && B8.size(1) >= Tp, "gemm_fp8_wgrad: operand too small");
  TORCH_CHECK(Tp % 128 == 0 && ksplit % 128 == 0 && K % 8 == 0, "gemm_fp8_wgrad: Tp, ksplit multiples of 128");
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == torch::kFloat32 && ws.dim() == 3 && ws.stride(2) == 1 && ws.size(1) >= N &&
                  ws.size(2) >= K && ws.size(0) >= (Tp + ksplit - 1) / ksplit,
              "gemm_fp8_wgrad: workspace [splits][N][K] f32");
  p.C = ws.data_ptr(); p.ldc = ws.stride(1); p.split_stride = ws.stride(0);
  p.scale_a = f32(scale_a, "scale_a"); p.scale_b = f32(scale_b, "scale_b");
  p.elem8 = 1; p.fmt_a = (int)fmt_a; p.fmt_b = 0;
  p.k_split_len = (int)ksplit;
  p.epi = 4;  // EPI_F32_STORE
  p.tile_cfg = 14;
  check(pvr_gemm(&p, stream()), "gemm_fp8_wgrad");
}

// y[rows][cols] (uint8 fp8) = sat(x * qscale); amax (int32 holding float bits) = max(amax, max|x|).
// y / qscale None: amax only.
void fp8_quant(torch::Tensor x, c10::optional<torch::Tensor> y, c10::optional<torch::Tensor> qscale, torch::Tensor amax, int64_t fmt) {
  const uint16_t* xp = bf(x, "x");
  const int64_t ldx = ld_of(x, "x");
  uint8_t* yp = nullptr;
  int64_t ldy = 0;
  if (y.has_value() && y->defined()) {
    yp = const_cast<uint8_t*>(u8(*y, "y"));
    ldy = y->stride(0);
    TORCH_CHECK(y->size(0) == x.size(0) && y->size(1) == x.size(1), "fp8_quant: shape mismatch");
  }
  TORCH_CHECK(amax.is_cuda() && amax.scalar_type() == torch::kInt32 && amax.numel() >= 1, "fp8_quant: amax int32");
  const float* qs = nullptr;
  if (qscale.has_value() && qscale->defined()) qs = f32(*qscale, "qscale");
  TORCH_CHECK(yp == nullptr || qs != nullptr, "fp8_quant: y needs qscale");
  check(pvr_fp8_quant(xp, ldx, yp, ldy, x.size(0), (int)x.size(1), qs, reinterpret_cast<unsigned*>(amax.data_ptr()), (int)fmt, stream()),
        "fp8_quant");
}

torch::Tensor fp8_dequant(torch::Tensor x, c10::optional<torch::Tensor> dscale, int64_t fmt) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kUInt8 && x.is_contiguous(), "fp8_dequant: contiguous uint8");
  auto y = torch::empty(x.sizes(), x.options().dtype(torch::kFloat32));
  const float* ds = nullptr;
  if (dscale.has_value() && dscale->defined()) ds = f32(*dscale, "dscale");
  check(pvr_fp8_dequant(x.data_ptr<uint8_t>(), y.data_ptr<float>(), x.numel(), ds, (int)fmt, stream()), "fp8_dequant");
  return y;
}

// multi-tensor weight quantization: segs = int64 [nseg][5] {src bf16 ptr, dst fp8 ptr, n, slot, first
// chunk} on the device (built once by the caller), nchunks = total chunks; amax_only: record max|x|
// per slot instead of quantizing
void fp8_quant_multi(torch::Tensor segs, int64_t nchunks, c10::optional<torch::Tensor> qscale, torch::Tensor amax, int64_t fmt,
                     bool amax_only) {
  TORCH_CHECK(segs.is_cuda() && segs.scalar_type() == torch::kInt64 && segs.dim() == 2 && segs.size(1) == 5 && segs.is_contiguous(),
              "fp8_quant_multi: segs int64 [n][5]");
  TORCH_CHECK(amax.is_cuda() && amax.scalar_type() == torch::kInt32, "fp8_quant_multi: amax int32");
  const float* qs = qscale.has_value() && qscale->defined() ? f32(*qscale, "qscale") : nullptr;
  TORCH_CHECK(amax_only || qs != nullptr, "fp8_quant_multi: quantizing needs qscale");
  check(pvr_fp8_quant_multi(segs.data_ptr<int64_t>(), (int)segs.size(0), nchunks, qs, reinterpret_cast<unsigned*>(amax.data_ptr()),
                            (int)fmt, amax_only ? 1 : 0, stream()),
        "fp8_quant_multi");
}

void fp8_scale_update(torch::Tensor hist, torch::Tensor amax, torch::Tensor qscale, torch::Tensor dscale, torch::Tensor fmax, int64_t s0,
                      int64_t s1, double margin_mul) {
  TORCH_CHECK(hist.dim() == 2 && hist.is_contiguous(), "hist [n][H]");
  TORCH_CHECK(amax.scalar_type() == torch::kInt32, "amax int32");
  TORCH_CHECK(s0 >= 0 && s1 <= hist.size(0), "slot range");
  check(pvr_fp8_scale_update(f32_mut(hist, "hist"), (int)hist.size(1), reinterpret_cast<unsigned*>(amax.data_ptr()), f32_mut(qscale, "qscale"),
                             f32_mut(dscale, "dscale"), f32(fmax, "fmax"), (int)s0, (int)s1, (float)margin_mul, stream()),
        "fp8_scale_update");
}

// seed / seed_offset / drop_p: attention-probability dropout (the backward gets the same three)
std::vector<torch::Tensor> attn_fwd(torch::Tensor qkv, int64_t B, int64_t N, int64_t H, double scale, c10::optional<torch::Tensor> seed,
                                    int64_t seed_offset, double drop_p, c10::optional<torch::Tensor> q_out,
                                    c10::optional<torch::Tensor> q_scale, c10::optional<torch::Tensor> q_amax, bool q_only) {
  const int64_t D = qkv.size(1) / 3;
  auto out = torch::empty({B * N, D}, qkv.options());
  auto lse = torch::empty({B * H, N}, qkv.options().dtype(torch::kFloat32));
  TORCH_CHECK(!q_only || (q_out.has_value() && q_out->defined()), "attn_fwd: q_only needs q_out");
  TORCH_CHECK(qkv.size(0) == B * N, "attn_fwd: qkv rows != B*N");
  const pvr::DropSite d = drop_args(seed, seed_offset, drop_p, "attn_fwd");
  // e4m3 copy of the output (producer-side quantization for an fp8 out-proj GEMM)
  const pvr::Fp8Copy q8 = fp8_copy(q_out, q_scale, q_amax, 0, B * N, D, 4, "attn_fwd");
  check(pvr_attn_fwd(bf(qkv, "qkv"), ld_of(qkv, "qkv"), bf_mut(out, "out"), D, f32_mut(lse, "lse"), (int)B, (int)N, (int)H, (int)D,
                     (float)scale, d, q8, q_only ? 1 : 0, stream()),
        "attn_fwd");
  return {out, lse};
}

// dbias[3D] += the in_proj bias gradient from the pipelined backward's [B*H][NQ][192] partials
// (per query block: dQ column sums of two query halves | dO column sums; the k slice gets none)
void attn_dbias_reduce(torch::Tensor part, int64_t B, int64_t H, torch::Tensor dbias) {
  TORCH_CHECK(dbias.is_cuda() && dbias.scalar_type() == torch::kFloat32 && dbias.is_contiguous() && dbias.numel() % (3 * H) == 0,
              "attn_dbias_reduce: f32 [3D] bias gradient");
  const int64_t DH = dbias.numel() / (3 * H);
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == torch::kFloat32 && part.is_contiguous() && part.numel() % (B * H * 3 * DH) == 0,
              "attn_dbias_reduce: f32 [B*H][R][3 * head dim] partials");
  const int64_t NQ = part.numel() / (B * H * 3 * DH);
  auto ws = torch::empty({(int64_t)pvr_attn_dbias_splits((int)B, (int)NQ) * H * 2 * DH}, part.options());
  check(pvr_attn_dbias_reduce(part.data_ptr<float>(), ws.data_ptr<float>(), dbias.data_ptr<float>(), (int)B, (int)H, (int)NQ,
                              (int)(DH * H), stream()),
        "attn_dbias_reduce");
}

// Persistent f32 dQ accumulator of the multi-key-block attention backward, one per (device, stream),
// zero-initialised once: the backward converts the accumulated dQ and zeroes it again, so no
// per-call zero fill (a 151 MB memset per layer at ViT-L/16 384 px). Deliberately never freed (a
// static tensor's destructor would run after the HIP runtime's teardown).
// drop = true: forget the cached accumulator of this (device, stream) (after a failed backward, whose
// partial sums it may still hold); the next call re-creates it with torch::zeros.
torch::Tensor dq_workspace(int64_t numel, const torch::TensorOptions& opts, bool drop = false) {
  DqWs& d = scratch_map<DqWs>()[scratch_key((int)opts.device().index())];
  if (drop) {
    d.t = torch::Tensor();
    return torch::Tensor();
  }
  // (a replaced tensor's memory returns to the caching allocator, stream-ordered)
  if (!d.t.defined() || d.t.numel() < numel) d.t = torch::zeros({numel}, opts.dtype(torch::kFloat32));
  return d.t;
}

// Scratch of the generic attention backward, one per (device, stream), grown to the largest request
// (never freed: see dq_workspace). Calls on one stream are serialised, so they share it.
torch::Tensor attn_scratch(int64_t numel, const torch::TensorOptions& opts) {
  AttnWs& d = scratch_map<AttnWs>()[scratch_key((int)opts.device().index())];
  if (!d.t.defined() || d.t.numel() < numel) d.t = torch::empty({numel}, opts.dtype(torch::kFloat32));
  return d.t;
}

// Release every per-(device, stream) scratch buffer above (split tails, split-K counters,
// deterministic partial rows, the attention backward's dQ accumulator and scratch) to the caching
// allocator. The caller makes sure no kernel still uses them (ops: _ext.free_scratch synchronizes
// first); the next call on a stream re-creates what it needs (counters zeroed again).
void free_scratch() {
  scratch_map<TailBufs>().clear();
  scratch_map<SkCounters>().clear();
  scratch_map<DetWs>().clear();
  scratch_map<DqWs>().clear();
  scratch_map<AttnWs>().clear();
}

// R > 0: for the standard layouts of this shape (qkv [T][3D], dO / O [T][D]) the backward emits the
// in_proj bias gradient as f32 [B*H][R][192] partials (pipelined or chunked kernel); 0: it does not
int64_t attn_bwd_bias_rows(int64_t B, int64_t N, int64_t H, int64_t D, bool drop) {
  return pvr_attn_bwd_part_rows((int)B, (int)N, (int)H, (int)D, 3 * D, D, D, 3 * D, drop ? 1 : 0);
}

// 1 if attn_bwd can write dQKV's e5m2 copy (q_out) for this shape with the standard layouts (the
// generic kernels write every final dQ value; not the pipelined ViT-B/16 kernel)
bool attn_bwd_q8_ok(int64_t B, int64_t N, int64_t H, int64_t D, bool drop) {
  return pvr_attn_bwd_q8_ok((int)N, drop ? 1 : 0) && !pvr_attn_bwd_uses_pipe((int)B, (int)N, (int)H, (int)D, 3 * D, D, D, 3 * D, drop ? 1 : 0);
}

// dbias: [3D] f32 accumulated with the in_proj bias gradient. dbias_part (pipelined path only,
// [B*H][ceil(N/32)][192] f32): receives the kernel's per-block partials instead, left unreduced (the
// caller reduces them, e.g. on the weight-gradient side stream: attn_dbias_reduce).
torch::Tensor attn_bwd(torch::Tensor dout, torch::Tensor qkv, torch::Tensor out, torch::Tensor lse, int64_t B, int64_t N, int64_t H,
                       double scale, c10::optional<torch::Tensor> dbias, c10::optional<torch::Tensor> dbias_part_out,
                       c10::optional<torch::Tensor> seed, int64_t seed_offset, double drop_p, c10::optional<torch::Tensor> q_out,
                       c10::optional<torch::Tensor> q_scale, c10::optional<torch::Tensor> q_amax, bool q_only,
                       int64_t q_fmt) {
  const int64_t D = qkv.size(1) / 3;
  auto dqkv = torch::empty_like(qkv);
  torch::Tensor dq_acc;
  int dq_rezero = 0;
  const pvr::DropSite drop = drop_args(seed, seed_offset, drop_p, "attn_bwd");
  const int has_drop = drop.seed ? 1 : 0;
  const int64_t dh = D / H;
  // fused in_proj bias gradient: per-(batch, head, row) partials written by the kernels (no atomics;
  // pipelined kernel: per 32-query block, generic kernel: one row per pair), reduced below
  torch::Tensor dbias_part, old_part;
  const bool want_db = dbias.has_value() && dbias->defined();
  const int64_t lds[4] = {ld_of(qkv, "qkv"), ld_of(dout, "dout"), ld_of(out, "out"), ld_of(dqkv, "dqkv")};
  const int prow = pvr_attn_bwd_part_rows((int)B, (int)N, (int)H, (int)D, lds[0], lds[1], lds[2], lds[3], has_drop);
  const bool parts = prow > 0;  // the kernels write [B*H][prow][3*dh] partials
  const bool pipe = pvr_attn_bwd_uses_pipe((int)B, (int)N, (int)H, (int)D, lds[0], lds[1], lds[2], lds[3], has_drop) != 0;
  const bool part_out = dbias_part_out.has_value() && dbias_part_out->defined();
  if (part_out) {
    TORCH_CHECK(parts && !want_db, "dbias_part: shapes with attn_bwd_bias_rows > 0 only, and not together with dbias");
    TORCH_CHECK(dbias_part_out->is_cuda() && dbias_part_out->scalar_type() == torch::kFloat32 && dbias_part_out->is_contiguous() &&
                    dbias_part_out->numel() == B * H * prow * 3 * dh,
                "dbias_part [B*H][attn_bwd_bias_rows][3 * head dim] f32");
    dbias_part = *dbias_part_out;
  }
  if (want_db) {
    TORCH_CHECK(dbias->numel() == 3 * D && dbias->scalar_type() == torch::kFloat32 && dbias->is_contiguous(), "dbias [3D] f32");
    if (parts)  // q sums of the two 16-query fragment rows | v sums, per (batch, head, row)
      dbias_part = torch::empty({B * H, (int64_t)prow, 3 * dh}, qkv.options().dtype(torch::kFloat32));
    else if (2 * (dh / 16) <= 2 * pvr_attn_bwd_waves((int)N))
      old_part = torch::empty({B * pvr_attn_bwd_key_blocks((int)N), 3 * D}, qkv.options().dtype(torch::kFloat32));
  }
  const int old_db = old_part.defined() ? 1 : 0;
  if (pvr_attn_bwd_needs_dq_acc((int)N, (int)dh, old_db, has_drop, g_deterministic ? 1 : 0)) {
    // several key blocks per head and neither the lastkey nor the tail-split slab path (e.g. N = 677):
    // dQ is summed with f32 atomics (deterministic mode: per-key-block slabs summed in order instead)
    dq_acc = dq_workspace(B * N * D, qkv.options());
    dq_rezero = dq_acc.defined() ? 1 : 0;
    if (!dq_acc.defined()) dq_acc = torch::zeros({B * N, D}, qkv.options().dtype(torch::kFloat32));
  }
  // optional e5m2 copy of dQKV + amax record (the fp8 recipe's dgrad / weight-gradient operand)
  const pvr::Fp8Copy q8 = fp8_copy(q_out, q_scale, q_amax, q_fmt, B * N, 3 * D, 4, "attn_bwd");
  if (q8.out)
    TORCH_CHECK(pvr_attn_bwd_q8_ok((int)N, has_drop) && !old_db && !pipe, "attn_bwd: no e5m2 dQKV copy for this shape (see attn_bwd_q8_ok)");
  // pre-pass outputs of the generic backward (per-query delta, lastkey path: ds_last; slab path: dQ
  // slabs): a persistent per-(device, stream) scratch, so the slab path (~0.9 GB per ViT-L/16@384
  // b128 layer) is not allocated on every backward
  auto ws = attn_scratch(pvr_attn_bwd_ws_floats((int)B, (int)N, (int)H, (int)D, old_db, has_drop, g_deterministic ? 1 : 0), qkv.options());
  pvr::AttnBwdParams p{};
  p.qkv = bf(qkv, "qkv"); p.ld = lds[0];
  p.out = bf(out, "out"); p.ld_o = lds[2];
  p.dout = bf(dout, "dout"); p.ld_do = lds[1];
  p.dqkv = bf_mut(dqkv, "dqkv"); p.ld_dq = lds[3];
  p.lse = f32(lse, "lse"); p.ws = ws.data_ptr<float>();
  p.dq_acc = dq_acc.defined() ? dq_acc.data_ptr<float>() : nullptr; p.dq_rezero = dq_rezero;
  p.dbias = pipe && dbias_part.defined() ? dbias_part.data_ptr<float>() : old_db ? old_part.data_ptr<float>() : nullptr;
  p.bpart = !pipe && dbias_part.defined() ? dbias_part.data_ptr<float>() : nullptr;
  p.B = (int)B; p.N = (int)N; p.H = (int)H; p.D = (int)D; p.scale = (float)scale;
  p.drop = drop; p.q8 = q8; p.q8_only = q_only && q8.out ? 1 : 0;
  const hipError_t err = pvr_attn_bwd(&p, stream());
  // a persistent accumulator is re-zeroed only by a completed backward: after a failed launch it
  // may hold stale partial sums, so it is dropped (re-created zeroed by the next call)
  if (err != hipSuccess && dq_rezero) dq_workspace(0, qkv.options(), true);
  check(err, "attn_bwd");
  if (want_db) {
    if (parts)
      attn_dbias_reduce(dbias_part, B, H, *dbias);
    else if (old_db)
      dbias->add_(old_part.sum(0));
    else
      dbias->add_(dqkv.sum(0, false, torch::kFloat32));
  }
  return dqkv;
}

// Class-token attention forward (csrc/attention.hip): qkv [B*N][3D] -> {o_0 [B][D] bf16, lse_0 [B*H] f32}
// of each image's token-0 query (no attention dropout)
std::vector<torch::Tensor> attn_cls_fwd(torch::Tensor qkv, int64_t B, int64_t N, int64_t H, double scale) {
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) == B * N && qkv.size(1) % 3 == 0 && H > 0, "attn_cls_fwd: qkv [B*N][3D]");
  const int64_t D = qkv.size(1) / 3;
  TORCH_CHECK(D % H == 0 && pvr_attn_cls_ok((int)N, (int)(D / H)), "attn_cls_fwd: unsupported N / head dim (attn_cls_ok)");
  auto out = torch::empty({B, D}, qkv.options());
  auto lse = torch::empty({B * H}, qkv.options().dtype(torch::kFloat32));
  check(pvr_attn_cls_fwd(bf(qkv, "qkv"), ld_of(qkv, "qkv"), bf_mut(out, "out"), D, f32_mut(lse, "lse"), (int)B, (int)N, (int)H, (int)D,
                         (float)scale, stream()),
        "attn_cls_fwd");
  return {out, lse};
}

// Class-token attention backward: returns {dqkv [B*N][3D] bf16 (dQ rows other than token 0 zero), dq0 [B][D]
// f32}; dbias [3D] f32 (optional) accumulates the in_proj bias gradient
std::vector<torch::Tensor> attn_cls_bwd(torch::Tensor dout, torch::Tensor qkv, torch::Tensor out, torch::Tensor lse, int64_t B, int64_t N,
                                        int64_t H, double scale) {
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) == B * N && qkv.size(1) % 3 == 0 && H > 0, "attn_cls_bwd: qkv [B*N][3D]");
  const int64_t D = qkv.size(1) / 3;
  TORCH_CHECK(D % H == 0 && pvr_attn_cls_ok((int)N, (int)(D / H)), "attn_cls_bwd: unsupported N / head dim (attn_cls_ok)");
  TORCH_CHECK(dout.dim() == 2 && dout.size(0) == B && dout.size(1) == D && out.dim() == 2 && out.size(0) == B && out.size(1) == D &&
                  lse.numel() == B * H && lse.is_contiguous(),
              "attn_cls_bwd: dout / out [B][D], lse [B*H]");
  auto dqkv = torch::empty({B * N, 3 * D}, qkv.options());
  auto dq0 = torch::empty({B, D}, qkv.options().dtype(torch::kFloat32));
  check(pvr_attn_cls_bwd(bf(qkv, "qkv"), ld_of(qkv, "qkv"), bf(out, "out"), ld_of(out, "out"), bf(dout, "dout"), ld_of(dout, "dout"),
                         f32(lse, "lse"), bf_mut(dqkv, "dqkv"), 3 * D, f32_mut(dq0, "dq0"), (int)B, (int)N, (int)H, (int)D, (float)scale,
                         stream()),
        "attn_cls_bwd");
  return {dqkv, dq0};
}

// dbias [3D] f32 += in_proj bias gradient of the class-token attention from dq0 [B][D] f32 and dout [B][D] bf16
void attn_cls_dbias(torch::Tensor dq0, torch::Tensor dout, torch::Tensor dbias) {
  TORCH_CHECK(dq0.dim() == 2 && dq0.is_contiguous() && dout.dim() == 2 && dout.size(0) == dq0.size(0) && dout.size(1) == dq0.size(1) &&
                  dbias.is_contiguous() && dbias.numel() == 3 * dq0.size(1),
              "attn_cls_dbias: dq0 f32 [B][D] contiguous, dout bf16 [B][D], dbias f32 [3D]");
  check(pvr_attn_cls_dbias(f32(dq0, "dq0"), bf(dout, "dout"), ld_of(dout, "dout"), f32_mut(dbias, "dbias"), (int)dq0.size(0),
                           (int)dq0.size(1), stream()),
        "attn_cls_dbias");
}

}  // namespace

extern "C" const char* pvr_src_hash(void);  // _build/src_hash.c (build.py): hash of csrc/*

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X (gfx950) HIP kernels for pytorch_vit_paper_replication_amd";
  m.def("source_hash", []() { return std::string(pvr_src_hash()); },
        "content hash of the csrc/ sources this binary was built from (build.source_hash())");
  m.def("gemm_tail_split", [](int64_t M, int64_t N, int64_t K, int64_t elem_bytes, int64_t max_units) {
    return pvr_gemm_tail_split((int)M, (int)N, (int)K, (int)elem_bytes, (int)max_units); },
    py::arg("M"), py::arg("N"), py::arg("K"), py::arg("elem_bytes"), py::arg("max_units") = 0,
    "K-parts of the split tail round this GEMM shape gets (0: none)");
  m.def("set_attn_dbg", [](torch::Tensor t) { pvr_set_attn_dbg(t.defined() && t.numel() ? t.data_ptr() : nullptr); },
        "diagnostic builds (-DPVR_ATTN_STAMPS): int64 buffer for the attention backward's phase stamps "
        "[workgroup * waves + wave][8] (scripts/attn_stamps.py); a no-op otherwise");
  m.def("set_attn_prep_xcd", &pvr_set_attn_prep_xcd, "attention backward pre-pass: XCD-contiguous (batch, head) pairs (1) or round-robin (0, default); A/B");
  m.def("set_ln_fwd_q8_grid", &pvr_set_ln_fwd_q8_grid, "LayerNorm forward with the e4m3 copy: grid cap in workgroups per CU (A/B)");
  m.def("set_attn_fwd_head_qf", &pvr_set_attn_fwd_head_qf, "whole-head attention forward (dh 64, N <= 256): 16-query fragments per wave (1 = default, 2 = half the LDS reads with 7 waves; A/B)");
  m.def("set_attn_fwd_qg", &pvr_set_attn_fwd_qg, "tiled attention forward: 16-query groups per wave (0 = auto by query padding, 1 = round-3 form, 2 = forced; A/B)");
  m.def("set_fp8_persistent", &pvr_set_fp8_persistent, "fp8 fwd/dgrad GEMMs on the persistent ping-pong: 1 when the epilogue has no per-row input (default), 0 never (A/B)");
  m.def("set_deterministic", &set_deterministic, "deterministic reductions (partial rows + ordered sum) instead of float atomics");
  m.def("deterministic", &deterministic);
  m.def("set_gemm_tail", &set_gemm_tail, "split-K tail of the last dispatch round on (True, default) / off (A/B)");
  m.def("set_gemm_lean", &set_gemm_lean,
        "lean GEMM instantiations on (True, default; PVR_GEMM_LEAN=0 at import: off) / off: every launch takes the general kernel");
  m.def("gemm_lean_last", [] { return (int64_t)pvr_gemm_lean_last(); },
        "GemmLean bits (csrc/gemm_lean.h) of the kernel the most recent gemm launched; 0: a general kernel");
  m.def("gemm", &gemm,py::arg("A"), py::arg("a_kcontig"), py::arg("B"), py::arg("b_kcontig"), py::arg("C"),
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("epi"), py::arg("bias"), py::arg("resid"), py::arg("addend"),
        py::arg("addend_period"), py::arg("aux"), py::arg("row_group"), py::arg("row_stride_group"),
        py::arg("row_offset"), py::arg("seed"), py::arg("seed_offset"), py::arg("drop_p"), py::arg("k_split"),
        py::arg("tile_cfg"), py::arg("dbg") = py::none(), py::arg("colsum") = py::none(),
        py::arg("epi_staged") = 0, py::arg("tail_limit") = 0, py::arg("reduce_out") = py::none(), py::arg("reduce_acc") = true,
        py::arg("drop_row_mul") = 0, py::arg("dp_seed") = py::none(), py::arg("dp_offset") = 0, py::arg("dp_p") = 0.0,
        py::arg("dp_rows") = 1);
  m.def("drop_path_scale", &drop_path_scale, py::arg("seed"), py::arg("site_offset"), py::arg("p"), py::arg("B"));
  m.def("splitk_timeouts", &splitk_timeouts, py::arg("like"), py::arg("reset") = false);
  m.def("num_cus", &num_cus);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("free_scratch", &free_scratch);
  m.def("layernorm_fwd_q8", &layernorm_fwd_q8);
  m.def("layernorm_bwd", &layernorm_bwd, py::arg("dy"), py::arg("dy_stride"), py::arg("x"), py::arg("x_stride"),
        py::arg("mean"), py::arg("rstd"), py::arg("w"), py::arg("dres"), py::arg("dres_stride"), py::arg("dx"),
        py::arg("dx_stride"), py::arg("dw"), py::arg("db"), py::arg("rows"), py::arg("dsum") = py::none(),
        py::arg("dz") = py::none(), py::arg("seed") = py::none(), py::arg("seed_offset") = 0, py::arg("drop_p") = 0.0,
        py::arg("q_out") = py::none(), py::arg("q_scale") = py::none(), py::arg("q_amax") = py::none(),
        py::arg("dz_nostore") = false, py::arg("q_fmt") = 1, py::arg("dres_every") = 0, py::arg("dp_seed") = py::none(),
        py::arg("dp_offset") = 0, py::arg("dp_p") = 0.0, py::arg("dp_rows") = 1);
  m.def("cast_f32_bf16", &cast_f32_bf16);
  m.def("splitk_epilogue", &splitk_epilogue);
  m.def("attn_bwd_bias_rows", &attn_bwd_bias_rows, py::arg("B"), py::arg("N"), py::arg("H"), py::arg("D"), py::arg("drop") = false);
  m.def("attn_dbias_reduce", &attn_dbias_reduce);
  m.def("splitk_reduce", &splitk_reduce);
  m.def("pad_cols_bf16", &pad_cols_bf16);
  m.def("transpose_batched", &transpose_batched);
  m.def("colsum", &colsum, py::arg("dy"), py::arg("rows"), py::arg("N"), py::arg("db"), py::arg("dz"), py::arg("seed"),
        py::arg("seed_offset"), py::arg("drop_p"), py::arg("q_out") = py::none(), py::arg("q_scale") = py::none(),
        py::arg("q_amax") = py::none(), py::arg("q_fmt") = 1, py::arg("row_mul") = 1, py::arg("dp_seed") = py::none(),
        py::arg("dp_offset") = 0, py::arg("dp_p") = 0.0, py::arg("dp_rows") = 1);
  m.def("im2col", &im2col, py::arg("img"), py::arg("out"), py::arg("P"), py::arg("Kp"), py::arg("mix") = py::none(),
        py::arg("mix_host") = py::none(), py::arg("keep") = py::none(), py::arg("erase") = py::none(),
        py::arg("erase_host") = py::none(), py::arg("erase_mode") = "const", py::arg("erase_value") = std::vector<double>{0.0},
        py::arg("erase_seed") = py::none(), py::arg("erase_offset") = 0);
  m.def("im2col_u8", &im2col_u8, py::arg("img"), py::arg("out"), py::arg("mean"), py::arg("std"), py::arg("geom"), py::arg("H"),
        py::arg("W"), py::arg("P"), py::arg("Kp"), py::arg("mix") = py::none(), py::arg("mix_host") = py::none(),
        py::arg("keep") = py::none(), py::arg("erase") = py::none(), py::arg("erase_host") = py::none(),
        py::arg("erase_mode") = "const", py::arg("erase_value") = std::vector<double>{0.0}, py::arg("erase_seed") = py::none(),
        py::arg("erase_offset") = 0);
  m.def("color_u8", &color_u8, py::arg("img"), py::arg("plan"), py::arg("plan_host") = py::none());
  m.def("erase_noise", &erase_noise, py::arg("seed"), py::arg("site_offset"), py::arg("B"), py::arg("C"), py::arg("H"), py::arg("W"));
  m.def("patch_keep_table", &patch_keep_table, py::arg("seed"), py::arg("site_offset"), py::arg("B"), py::arg("n_p"), py::arg("n_keep"));
  m.def("pos_gather", &pos_gather, py::arg("pos"), py::arg("keep"));
  m.def("cls_rows", &cls_rows);
  m.def("patch_bwd", &patch_bwd, py::arg("dE"), py::arg("B"), py::arg("ntok"), py::arg("D"), py::arg("dpos"), py::arg("dcls"),
        py::arg("dconv"), py::arg("dbias"), py::arg("seed"), py::arg("seed_offset"), py::arg("drop_p"), py::arg("inv") = py::none(),
        py::arg("n_keep") = 0);
  m.def("xent", &xent, py::arg("logits"), py::arg("labels"), py::arg("dlogits"), py::arg("correct"), py::arg("grad_scale"),
        py::arg("mean") = py::none());
  m.def("xent_soft", &xent_soft, py::arg("logits"), py::arg("ya"), py::arg("yb"), py::arg("lam"), py::arg("eps"),
        py::arg("dlogits"), py::arg("correct"), py::arg("grad_scale"), py::arg("mean") = py::none());
  m.def("bce", &bce, py::arg("logits"), py::arg("ya"), py::arg("yb"), py::arg("lam"), py::arg("eps"), py::arg("thr"),
        py::arg("sum_classes"), py::arg("dlogits"), py::arg("correct"), py::arg("grad_scale"), py::arg("mean") = py::none());
  m.def("grad_norm", &grad_norm);
  m.def("norm_partial_blocks", []() { return pvr_norm_partial_blocks(); });
  m.def("adam", &adam, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("shadow"), py::arg("seg_start"),
        py::arg("seg_group"), py::arg("groups"), py::arg("clip"), py::arg("skip_nonfinite"), py::arg("ema") = py::none(),
        py::arg("ema_pair") = py::none());
  m.def("adam_t", &adam_t, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("shadow"), py::arg("shadow_t"),
        py::arg("tmeta"), py::arg("ntiles"), py::arg("fmeta"), py::arg("flat4"), py::arg("groups"), py::arg("clip"),
        py::arg("skip_nonfinite"), py::arg("ema") = py::none(), py::arg("ema_pair") = py::none());
  m.def("lamb_chunk", []() { return (int)pvr::LAMB_CHUNK; });
  m.def("lamb_moments", &lamb_moments, py::arg("p"), py::arg("g"), py::arg("m"), py::arg("v"), py::arg("chunks"), py::arg("seg_group"),
        py::arg("partial"), py::arg("groups"), py::arg("clip"), py::arg("skip_nonfinite"));
  m.def("lamb_ratio", &lamb_ratio, py::arg("partial"), py::arg("seg_chunks"), py::arg("seg_group"), py::arg("trust"), py::arg("groups"),
        py::arg("clip"), py::arg("skip_nonfinite"));
  m.def("lamb_update", &lamb_update, py::arg("p"), py::arg("m"), py::arg("v"), py::arg("shadow"), py::arg("trust"), py::arg("groups"),
        py::arg("clip"), py::arg("skip_nonfinite"), py::arg("seg_start") = py::none(), py::arg("seg_group") = py::none(),
        py::arg("shadow_t") = py::none(), py::arg("tmeta") = py::none(), py::arg("ntiles") = 0, py::arg("fmeta") = py::none(),
        py::arg("flat4") = 0, py::arg("ema") = py::none(), py::arg("ema_pair") = py::none());
  py::class_<SgdTables>(m, "SgdTables", "host-checked segment or tile tables of the SGD kernels (sgd_segments / sgd_tiles)")
      .def_readonly("tiles", &SgdTables::tiles)
      .def_readonly("ntiles", &SgdTables::ntiles)
      .def_readonly("flat4", &SgdTables::flat4)
      .def_readonly("numel", &SgdTables::n);
  m.def("sgd_blocks", []() { return pvr_sgd_blocks(); });
  m.def("sgd_segments", &sgd_segments, py::arg("seg_start"), py::arg("seg_group"), py::arg("numel"), py::arg("device"));
  m.def("sgd_tiles", &sgd_tiles, py::arg("tmeta"), py::arg("fmeta"), py::arg("numel"), py::arg("numel_t"), py::arg("device"));
  m.def("sgd", &sgd, py::arg("p"), py::arg("g"), py::arg("buf"), py::arg("shadow"), py::arg("tables"), py::arg("groups"),
        py::arg("clip"), py::arg("skip_nonfinite"), py::arg("ema") = py::none(), py::arg("ema_pair") = py::none());
  m.def("sgd_t", &sgd_t, py::arg("p"), py::arg("g"), py::arg("buf"), py::arg("shadow"), py::arg("shadow_t"), py::arg("tables"),
        py::arg("groups"), py::arg("clip"), py::arg("skip_nonfinite"), py::arg("ema") = py::none(), py::arg("ema_pair") = py::none());
  m.def("scale_by_clip", &scale_by_clip);
  m.def("head_fwd", &head_fwd);
  m.def("head_bwd", &head_bwd, py::arg("dlogits"), py::arg("xhat"), py::arg("rstd"), py::arg("gamma"), py::arg("beta"), py::arg("W"),
        py::arg("B"), py::arg("N"), py::arg("dW") = py::none(), py::arg("db") = py::none(), py::arg("dgamma") = py::none(),
        py::arg("dbeta") = py::none());
  m.def("scale_by", &scale_by);
  m.def("metrics_accum", &metrics_accum);
  m.def("rng_next", &rng_next);
  m.def("zero_f32", &zero_f32);
  m.def("layerscale_fold", &layerscale_fold, py::arg("master"), py::arg("w16"), py::arg("wt16"), py::arg("bhat"), py::arg("meta"),
        py::arg("meta_host"));
  m.def("layerscale_unfold", &layerscale_unfold, py::arg("dw_hat"), py::arg("db_hat"), py::arg("W"), py::arg("b"), py::arg("g"),
        py::arg("gW") = py::none(), py::arg("gb") = py::none(), py::arg("gg") = py::none());
  m.def("gemm_fp8", &gemm_fp8, py::arg("A"), py::arg("fmt_a"), py::arg("B"), py::arg("fmt_b"), py::arg("C"), py::arg("M"),
        py::arg("N"), py::arg("K"), py::arg("epi"), py::arg("scale_a"), py::arg("scale_b"), py::arg("bias") = py::none(),
        py::arg("resid") = py::none(), py::arg("aux") = py::none(), py::arg("seed") = py::none(), py::arg("seed_offset") = 0,
        py::arg("drop_p") = 0.0, py::arg("colsum") = py::none(), py::arg("q_out") = py::none(), py::arg("q_scale") = py::none(),
        py::arg("q_amax") = py::none(), py::arg("q_fmt") = 0, py::arg("c_skip") = false, py::arg("tail_limit") = 0);
  m.def("fp8_transpose", &fp8_transpose);
  m.def("gemm_fp8_wgrad_mn", &gemm_fp8_wgrad_mn, py::arg("dy8"), py::arg("x8"), py::arg("ws"), py::arg("N"), py::arg("K"),
        py::arg("T"), py::arg("scale_a"), py::arg("scale_b"), py::arg("ksplit"), py::arg("fmt_a") = 1);
  m.def("fp8_quant", &fp8_quant, py::arg("x"), py::arg("y"), py::arg("qscale"), py::arg("amax"), py::arg("fmt"));
  m.def("fp8_dequant", &fp8_dequant, py::arg("x"), py::arg("dscale") = py::none(), py::arg("fmt") = 0);
  m.def("fp8_scale_update", &fp8_scale_update);
  m.def("fp8_quant_t", &fp8_quant_t);
  m.def("gemm_fp8_wgrad", &gemm_fp8_wgrad, py::arg("A8"), py::arg("B8"), py::arg("ws"), py::arg("N"), py::arg("K"), py::arg("Tp"),
        py::arg("scale_a"), py::arg("scale_b"), py::arg("ksplit"), py::arg("fmt_a") = 1);
  m.def("fp8_quant_multi", &fp8_quant_multi, py::arg("segs"), py::arg("nchunks"), py::arg("qscale"), py::arg("amax"), py::arg("fmt"),
        py::arg("amax_only"));
  m.def("attn_fwd", &attn_fwd, py::arg("qkv"), py::arg("B"), py::arg("N"), py::arg("H"), py::arg("scale"),
        py::arg("seed") = py::none(), py::arg("seed_offset") = 0, py::arg("drop_p") = 0.0, py::arg("q_out") = py::none(),
        py::arg("q_scale") = py::none(), py::arg("q_amax") = py::none(), py::arg("q_only") = false);
  m.def("attn_bwd", &attn_bwd, py::arg("dout"), py::arg("qkv"), py::arg("out"), py::arg("lse"), py::arg("B"), py::arg("N"),
        py::arg("H"), py::arg("scale"), py::arg("dbias") = py::none(), py::arg("dbias_part") = py::none(),
        py::arg("seed") = py::none(), py::arg("seed_offset") = 0, py::arg("drop_p") = 0.0, py::arg("q_out") = py::none(),
        py::arg("q_scale") = py::none(), py::arg("q_amax") = py::none(), py::arg("q_only") = false,
        py::arg("q_fmt") = 1);
  m.def("attn_cls_ok", [](int64_t N, int64_t dh) { return pvr_attn_cls_ok((int)N, (int)dh) != 0; },
        "the class-token attention kernels take this token count and head dim");
  m.def("attn_cls_fwd", &attn_cls_fwd, py::arg("qkv"), py::arg("B"), py::arg("N"), py::arg("H"), py::arg("scale"));
  m.def("attn_cls_bwd", &attn_cls_bwd, py::arg("dout"), py::arg("qkv"), py::arg("out"), py::arg("lse"), py::arg("B"), py::arg("N"),
        py::arg("H"), py::arg("scale"));
  m.def("attn_cls_dbias", &attn_cls_dbias);
  m.def("attn_bwd_q8_ok", &attn_bwd_q8_ok, "attn_bwd can write dQKV's e5m2 copy for this shape");
  m.def("arch", []() { return std::string("gfx950"); });
}
