// Host helpers every GEMM launcher uses (gemm_store.hip, gemm_recon.hip, gemm_mask.hip): operand
// checks, the option reads, LDS-attribute launches and capped grids.
#pragma once
#include "gemm_core.hpp"

namespace gm2 {

template <typename T>
static void check_gemm(const GemmArgs<T>& g, int tile) {
  if (g.K % kKPad || g.Mp % tile || g.Np % tile || g.M > g.Mp || g.N > g.Np || g.M <= 0 || g.N <= 0)
    throw Gm2Error("gemm: bad dims M=%d N=%d K=%d Mp=%d Np=%d (tile %d)", g.M, g.N, g.K, g.Mp, g.Np, tile);
  if ((g.pk ? g.ldp < g.K : g.ldp < g.Mp) || (g.qk ? g.ldq < g.K : g.ldq < g.Np)) throw Gm2Error("gemm: ld too small");
  if (((uintptr_t)g.P | (uintptr_t)g.Q) & 15) throw Gm2Error("gemm: operands not 16-B aligned");
  if ((g.ldp * sizeof(T)) % 16 || (g.ldq * sizeof(T)) % 16) throw Gm2Error("gemm: ld not 16-B multiple");
  if (tile == 256 && (g.ldp >= pp::kPPMaxLd || g.ldq >= pp::kPPMaxLd))  // (stage_half's 32-bit thread offsets)
    throw Gm2Error("gemm: row pitch %lld / %lld beyond the 256x256 tiles' limit", (long long)g.ldp, (long long)g.ldq);
}

// Main-loop selection for the 256x256 bf16 tiles: the ping-pong loop (default; measured
// +15-20 % on the long-K GEMMs of the v0 step, profiles/r02_gemm_bench.txt) or the two-stage loop
// (option GM2_OPT_GEMM_PP = 0, or env GM2_GEMM_PP=0 for the process defaults); both parity-tested.
static bool pp_enabled() { return opts().gemm_pp != 0; }

// call f(Cfg{}) with the 128x128 fp32-store tile configuration the options select: waves per block
// (GM2_OPT_SMALL_WAVES: 4 or 8; 8: step 3.52 -> 3.46 ms, profiles/r02_ab_small_waves.txt)
// (round 6 measured a 4-wave, 2-stage form with two workgroups per CU -- GM2_OPT_SMALL_PAIR, commits
// a952803 / 09afbbc -- neutral to slower at step level and removed it: profiles/r06_small_pair_ab.txt)
template <typename T, class F>
static auto small_cfg(F&& f) {
  return opts().small_waves == 8 ? f(SmallDeep8{}) : f(SmallDeep{});
}

// GM2_OPT_GRID_CAP bits: 1 = the output-layer weight-gradient GEMM (side stream, beside the
// hidden-layer backward chain), 2 = the input-layer one (beside the side stream's last hidden-layer
// weight gradients) on a capped grid -- same rounds, the last round's idle CUs free for the rest
// (default 2, dWe0 only: -18 us/step; bit 1 (dW9) measured 20-40 us/step slower: the chain's
// 256-tile GEMMs get 41 CUs (6 rounds) while dW9 runs, profiles/r02_grid_cap_ab_*)
static int grid_cap_bits() { return opts().grid_cap; }

// one launch with `lds` bytes of dynamic LDS, of a kernel whose launches take up to `lds_max`
template <class K, class... A>
static void launch_lds(K kernel, int grid, int threads, int lds_max, int lds, hipStream_t s, const A&... args) {
  ensure_lds_attr((const void*)kernel, lds_max);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds, s, args...);
}

// packed-bits output rows [m][ldb] that must cover `genes` bits
static void check_bits_pitch(const uint8_t* bits, int64_t ldb, int genes) {
  if (bits && ((ldb & 15) || (((uintptr_t)bits) & 15) || ldb * 8 < genes))
    throw Gm2Error("mask bits: row pitch %lld must be a multiple of 16 bytes covering the padded genes", (long long)ldb);
}

// workgroups of a launch over `tiles` tiles: all of them, or with GM2_OPT_GRID_CAP bit `bit` the
// capped grid of the same rounds
static GridCap grid_for(int tiles, int bit) {
  return (grid_cap_bits() & bit) ? capped_grid(tiles, device_cus()) : GridCap{tiles, 0};
}

}  // namespace gm2
