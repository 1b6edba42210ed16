// Host checks of the lean-instantiation chooser (csrc/gemm_lean.h) the GEMM launcher runs: the launches
// of the default ViT step on its list get their lean kernel, and every option a lean kernel does not carry
// (diagnostic stamps, fp8, drop path, addend, row groups, N % 8, the staged epilogue, c_skip, the
// in-launch split-K reduction, 64-bit dropout indices, option sets outside the list) falls back to
// the general kernel (0). Built and run by tests/test_gemm_lean_cpp.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pytorch_vit_paper_replication_amd/csrc/gemm_lean.h"

using namespace pvr;

static int failures = 0;
#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

// any non-null pointer: the chooser only tests pointers, it never reads through them
static float f32_[4];
static uint16_t bf_[4];
static uint64_t seed_[1];

// a k-contiguous bf16 forward launch of ViT-B/16 at batch 256
static GemmParams fwd(int epi, int N = 768, int K = 768) {
  GemmParams p{};
  p.M = 50432; p.N = N; p.K = K;
  p.lda = K; p.ldb = K; p.ldc = N;
  p.a_kcontig = p.b_kcontig = 1;
  p.k_split_len = K;
  p.epi = epi;
  p.drop_scale = 1.f;
  return p;
}
static void with_bias(GemmParams& p) { p.bias = f32_; }
static void with_resid(GemmParams& p) { p.resid = bf_; p.ld_resid = p.N; }
static void with_drop(GemmParams& p) { p.seed_ptr = seed_; p.drop_thr = 6554; p.drop_scale = 1.f / 0.9f; }
static void with_aux(GemmParams& p) { p.aux = bf_; p.ld_aux = p.N; }

constexpr int RBD = LEAN_ON | LEAN_BIAS | LEAN_RES | LEAN_DROP;

static void check_one_tile() {
  for (int tail = 0; tail < 2; ++tail) {
    const int t = tail ? LEAN_TAIL : 0;
    GemmParams out = fwd(0);
    with_bias(out); with_resid(out);
    CHECK(lean_choose(out, LEAN_K_ONE_TILE, tail) == 0);  // out-proj forward: measured no faster, general
    GemmParams fc2 = out;
    with_drop(fc2);
    CHECK(lean_choose(fc2, LEAN_K_ONE_TILE, tail) == (RBD | t));  // fc2 forward
    const GemmParams dgrad = fwd(0);
    CHECK(lean_choose(dgrad, LEAN_K_ONE_TILE, tail) == 0);  // plain dgrads: measured no faster, general
  }
  // option sets outside the list
  GemmParams p = fwd(0);
  with_bias(p);
  CHECK(lean_choose(p, LEAN_K_ONE_TILE, false) == 0);  // bias without a residual
  p = fwd(0);
  with_resid(p);
  CHECK(lean_choose(p, LEAN_K_ONE_TILE, false) == 0);  // residual without a bias
  p = fwd(0);
  with_drop(p);
  CHECK(lean_choose(p, LEAN_K_ONE_TILE, false) == 0);  // dropout alone
  p = fwd(1);
  with_bias(p);
  CHECK(lean_choose(p, LEAN_K_ONE_TILE, false) == 0);  // one-tile GELU / dGELU stay general
  p = fwd(2);
  with_aux(p);
  CHECK(lean_choose(p, LEAN_K_ONE_TILE, false) == 0);
}

// every option the lean kernels do not carry sends the launch to the general kernel
static void check_fallbacks(int kernel, const GemmParams& base, int want) {
  CHECK(lean_choose(base, kernel, false) == want);
  std::vector<GemmParams> v;
  GemmParams p = base;
  p.dbg = seed_; v.push_back(p);
  p = base; p.elem8 = 1; v.push_back(p);
  p = base; p.dp_thr = 100; v.push_back(p);
  p = base; p.drop_row_mul = 197; v.push_back(p);
  p = base; p.addend = f32_; p.addend_period = 197; v.push_back(p);
  p = base; p.row_group = 196; v.push_back(p);
  p = base; p.N = 772; v.push_back(p);
  p = base; p.epi_staged = 1; v.push_back(p);
  p = base; p.c_skip = 1; v.push_back(p);
  p = base; p.q_out = reinterpret_cast<uint8_t*>(bf_); v.push_back(p);
  p = base; p.k_split_len = base.K / 2; v.push_back(p);
  p = base; p.b_kcontig = 0; v.push_back(p);
  p = base; p.M = 1 << 21; p.ldc = 1024; v.push_back(p);  // M * ldc * 2 >= 2^31: buffer offsets
  for (const GemmParams& q : v) CHECK(lean_choose(q, kernel, false) == 0);
  if (base.drop_thr) {
    p = base; p.M = 6000000; v.clear();  // M * N + 8 > 2^32 - 1: the 64-bit hash, general kernel
    CHECK((uint64_t)p.M * (uint64_t)p.N + 8 > 0xFFFFFFFFull);
    CHECK(lean_choose(p, kernel, false) == 0);
    p = base; p.seed_ptr = nullptr;
    CHECK(lean_choose(p, kernel, false) == 0);
  }
}

static void check_persistent() {
  GemmParams qkv = fwd(0, 2304);
  with_bias(qkv);
  check_fallbacks(LEAN_K_PERSISTENT, qkv, LEAN_ON | LEAN_BIAS);
  GemmParams fc1 = fwd(1, 3072);
  with_bias(fc1); with_drop(fc1); with_aux(fc1);
  check_fallbacks(LEAN_K_PERSISTENT, fc1, LEAN_ON | LEAN_BIAS | LEAN_DROP | LEAN_AUX);
  GemmParams dg = fwd(2, 3072);
  with_aux(dg); dg.colsum = f32_;
  check_fallbacks(LEAN_K_PERSISTENT, dg, LEAN_ON | LEAN_AUX | LEAN_COLSUM);
  // outside the list: GELU without dropout / aux, dGELU without column sums, a residual, a tail
  GemmParams p = fc1; p.drop_thr = 0;
  CHECK(lean_choose(p, LEAN_K_PERSISTENT, false) == 0);
  p = fc1; p.aux = nullptr; p.ld_aux = 0;
  CHECK(lean_choose(p, LEAN_K_PERSISTENT, false) == 0);
  p = dg; p.colsum = nullptr;
  CHECK(lean_choose(p, LEAN_K_PERSISTENT, false) == 0);
  p = qkv; with_resid(p);
  CHECK(lean_choose(p, LEAN_K_PERSISTENT, false) == 0);
  CHECK(lean_choose(qkv, LEAN_K_PERSISTENT, true) == 0);
}

// the weight gradient's partial stores (mn-contiguous operands, EPI_F32_STORE) have no lean kernel
static void check_wgrad() {
  GemmParams w{};
  w.M = 768; w.N = 768; w.K = 50432;
  w.lda = 768; w.ldb = 768; w.ldc = 768;
  w.k_split_len = 1792; w.epi = 4; w.tile_cfg = 14; w.split_stride = 768 * 768;
  CHECK(lean_choose(w, LEAN_K_ONE_TILE, false) == 0);
  CHECK(lean_choose(w, LEAN_K_PERSISTENT, false) == 0);
}

int main() {
  check_one_tile();
  GemmParams fc2 = fwd(0, 768, 3072);
  with_bias(fc2); with_resid(fc2); with_drop(fc2);
  check_fallbacks(LEAN_K_ONE_TILE, fc2, RBD);
  check_persistent();
  check_wgrad();
  if (failures) {
    std::fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
