// Host checks of the host-kernel interface header (csrc/kernels.h) under the plain host compiler:
// it needs no device compiler, pvr::AdamGroup is exactly one float32 [10] row of the param-group table
// that optim/adam.py writes (argv[1]: two such rows, written by FusedAdam._group_array), and the
// argument structs that cross the boundary by value are trivially copyable.
// Built and run by tests/test_kernels_h_cpp.py.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "../../pytorch_vit_paper_replication_amd/csrc/kernels.h"

using namespace pvr;

static int failures = 0;
#define CHECK(c)                                                              \
  do {                                                                        \
    if (!(c)) {                                                               \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

static_assert(sizeof(AdamGroup) == 40 && alignof(AdamGroup) == 4 && ADAM_GROUP_COLS == 10, "one float32 [10] row");
static_assert(offsetof(AdamGroup, lr) == 0 && offsetof(AdamGroup, beta1) == 4 && offsetof(AdamGroup, beta2) == 8 &&
                  offsetof(AdamGroup, eps) == 12 && offsetof(AdamGroup, weight_decay) == 16 && offsetof(AdamGroup, bc1) == 20 &&
                  offsetof(AdamGroup, bc2_sqrt) == 24 && offsetof(AdamGroup, decoupled) == 28 &&
                  offsetof(AdamGroup, one_minus_beta1) == 32 && offsetof(AdamGroup, one_minus_beta2) == 36,
              "columns 0..9 of the group table");
static_assert(std::is_trivially_copyable<AdamGroup>::value && std::is_standard_layout<AdamGroup>::value, "AdamGroup");
static_assert(std::is_trivially_copyable<DropSite>::value && std::is_standard_layout<DropSite>::value, "DropSite");
static_assert(std::is_trivially_copyable<Fp8Copy>::value && std::is_standard_layout<Fp8Copy>::value, "Fp8Copy");
static_assert(std::is_trivially_copyable<LnBwdParams>::value && std::is_trivially_copyable<AttnBwdParams>::value &&
                  std::is_trivially_copyable<GemmParams>::value,
              "parameter structs");

int main(int argc, char** argv) {
  // a default site / copy means "none"
  const DropSite d{};
  const Fp8Copy q{};
  CHECK(d.seed == nullptr && d.offset == 0 && d.thr == 0 && d.scale == 1.f);
  CHECK(q.out == nullptr && q.ld == 0 && q.scale == nullptr && q.amax == nullptr && q.fmt == 0);

  // the rows FusedAdam._group_array wrote: lr 2 / 3, betas (0.375, 0.75), eps 0.125, weight decay
  // 0.0625 / 0, step 1 (bc1 = 0.625, bc2_sqrt = 0.5), decoupled 1 / 0
  if (argc < 2) {
    std::fprintf(stderr, "usage: test_kernels_h <group table file>\n");
    return 2;
  }
  float rows[21];
  std::FILE* f = std::fopen(argv[1], "rb");
  CHECK(f != nullptr);
  if (f) {
    CHECK(std::fread(rows, sizeof(float), 21, f) == 20);  // exactly two rows of 10
    std::fclose(f);
    AdamGroup g[2];
    std::memcpy(g, rows, sizeof(g));  // what bindings.cpp's reinterpret_cast reads
    CHECK(g[0].lr == 2.f && g[0].beta1 == 0.375f && g[0].beta2 == 0.75f && g[0].eps == 0.125f);
    CHECK(g[0].weight_decay == 0.0625f && g[0].bc1 == 0.625f && g[0].bc2_sqrt == 0.5f && g[0].decoupled == 1);
    CHECK(g[1].lr == 3.f && g[1].beta1 == 0.375f && g[1].beta2 == 0.75f && g[1].eps == 0.125f);
    CHECK(g[1].weight_decay == 0.f && g[1].bc1 == 0.625f && g[1].bc2_sqrt == 0.5f && g[1].decoupled == 0);
    for (int i = 0; i < 2; ++i) CHECK(g[i].one_minus_beta1 == 0.625f && g[i].one_minus_beta2 == 0.25f);
  }
  if (failures) return 1;
  std::puts("all checks passed");
  return 0;
}
