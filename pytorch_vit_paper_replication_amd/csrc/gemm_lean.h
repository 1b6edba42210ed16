// Lean instantiations of the 256x256 ping-pong GEMM kernels (csrc/gemm.hip), chosen on the host, as
// plain constexpr C++ (no HIP headers; tests/cpp/test_gemm_lean.cpp checks the chooser on the host).
//
// The general kernels are compiled once for every option a launch could ask for and test the options
// at run time (bias, dropout, residual, split tail, in-launch split-K reduction, diagnostic stamps,
// the fp8 forms' output copy). A lean instantiation carries the wave-uniform options of one launch
// kind of the default training step as template bits, has exactly one epilogue body and none of the
// other code. lean_choose() names the instantiation a launch matches, or 0: the general kernel, which
// stays the fallback for every shape and option the list below does not name.
#pragma once
#include "gemm_params.h"

namespace pvr {

enum GemmLean : int {
  LEAN_ON = 1,       // a lean instantiation (0: the general kernel)
  LEAN_BIAS = 2,     // p.bias is set
  LEAN_DROP = 4,     // p.drop_thr != 0, every element index below 2^32 (the 32-bit hash)
  LEAN_RES = 8,      // p.resid is set
  LEAN_TAIL = 16,    // the launch has a split tail: only these hold tail_gather / tail_sum
  LEAN_AUX = 32,     // p.aux is set (GELU: derivative store, dGELU: factor load)
  LEAN_COLSUM = 64,  // p.colsum is set (dGELU)
};

// which kernel the launch is about to take
enum GemmLeanKernel : int {
  LEAN_K_ONE_TILE = 0,    // gemm_pp_kernel<true, true, true, EPI>: one tile per workgroup, bf16 output
  LEAN_K_PERSISTENT = 1,  // gemm_ppp_kernel<true, EPI, true>: register-direct persistent form
};

// epilogue_direct's preconditions: plain row mapping, 16-B column groups, 31-bit buffer offsets
constexpr bool direct_ok_c(const GemmParams& p) {
  const int64_t l1 = p.ldc > p.ld_resid ? p.ldc : p.ld_resid;
  const int64_t ld = l1 > p.ld_aux ? l1 : p.ld_aux;
  return !p.addend && !p.row_group && (p.N & 7) == 0 && (int64_t)p.M * ld * 2 < (1ll << 31);
}

// The lean instantiation (GemmLean bits) of a bf16-operand launch on `kernel`, 0 for the general one.
// `tail`: the launch was planned with a split tail (one-tile kernel only). The list is the launches
// of the default ViT step whose lean kernel measured faster than the general one at its ViT-B/16
// batch-256 shape (profiles/gemm_lean/README.md):
//   one tile, EPI_BF16 (0), register-direct: residual + bias + dropout (fc2 forward), with and without
//     LEAN_TAIL;
//   persistent: EPI_BF16 with bias (qkv forward) | EPI_GELU (1) with bias + dropout + aux (fc1
//     forward) | EPI_DGELU (2) with aux + column sums (fc2 dgrad).
// Measured no faster, and left on the general kernels: the one-tile residual + bias form (out-proj
// forward), the one-tile form without bias / residual / dropout (plain dgrads) and the weight
// gradient's partial stores.
constexpr int lean_choose(const GemmParams& p, int kernel, bool tail) {
  if (p.dbg || p.elem8 || p.dp_thr || p.drop_row_mul) return 0;  // stamps, fp8, drop path: general
  if (!p.a_kcontig || !p.b_kcontig || p.epi_staged || p.c_skip || p.q_out || !direct_ok_c(p) || p.k_split_len < p.K) return 0;
  const bool bias = p.bias != nullptr, res = p.resid != nullptr, aux = p.aux != nullptr, cs = p.colsum != nullptr;
  const bool drop = p.drop_thr != 0;
  // a launch whose dropout index space needs 64 bits takes the general kernel
  if (drop && (!p.seed_ptr || (uint64_t)p.M * (uint64_t)p.N + 8 > 0xFFFFFFFFull)) return 0;
  if (kernel == LEAN_K_ONE_TILE) {
    if (p.epi != 0) return 0;
    if (bias && res && drop) return LEAN_ON | LEAN_BIAS | LEAN_RES | LEAN_DROP | (tail ? LEAN_TAIL : 0);
    return 0;
  }
  if (kernel == LEAN_K_PERSISTENT && !tail) {
    if (p.epi == 0 && bias && !res && !drop) return LEAN_ON | LEAN_BIAS;
    if (p.epi == 1 && bias && drop && aux) return LEAN_ON | LEAN_BIAS | LEAN_DROP | LEAN_AUX;
    if (p.epi == 2 && aux && cs) return LEAN_ON | LEAN_AUX | LEAN_COLSUM;
  }
  return 0;
}

}  // namespace pvr
