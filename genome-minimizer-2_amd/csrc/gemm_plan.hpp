// Launch geometry of the GEMM path: the host-side rules the launchers (gemm_*.hip) and their callers
// (api.hip) share, each stated once. Plain C++17: no HIP calls, no options, no device queries, so
// tools/asan/host_asan.cpp checks every rule against a table of expected values without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <stdexcept>

namespace gm2 {

struct GemmPlan {
  int tile, splits;
};

// Tile / split-K plan of C [Mp][Np] over K, elements of esize bytes (one K-tile = a 128-byte row
// chunk: 64 bf16 / 32 f32). Big tiles when they alone fill the chip, or when K is long enough that
// a split-K slab round trip is cheap next to the work; otherwise the 128-tile, split only when it
// leaves most CUs idle (and never below 8 K-steps per slice).
// (the exact-fp32 path stays on the 128x128 tiles: its K-step partial sums double the accumulator
// registers, which the 256x256 tile's 8 waves cannot hold)
// small_split (GM2_OPT_SMALL_SPLIT): split-K factor for the 128-tile GEMMs that alone fill the chip
// with one short-K tile per CU, the hidden-layer GEMMs (256 tiles, 16 K-steps): > 1 puts that many
// tiles on each CU so one's loads hide behind another's MFMAs; default 1
inline GemmPlan plan_gemm_dims(int esize, int Mp, int Np, int K, int small_split) {
  const int nk = K / (128 / esize);
  const int tiles_big = (esize == 2 && Mp % 256 == 0 && Np % 256 == 0) ? (Mp / 256) * (Np / 256) : 0;
  const int tiles_small = (Mp / 128) * (Np / 128);
  // (up to 32 K-slices: a launch with a few tiles -- the small-batch plans, e.g. the input layer and
  // the output layer's input gradient at batch 32 / 64: 8 tiles of 128 x 128 over K = 55,040 --
  // fills the chip; at most 8 had left 192 CUs idle, 117 -> ~30 us each at batch 64; the split
  // slabs are summed in slice order by their consumers, deterministic)
  auto cap = [&](int s) { return std::max(1, std::min({s, 32, std::max(1, nk / 8)})); };
  if (tiles_big >= 256) return {256, 1};
  if (tiles_big > 0 && K >= 8192) return {256, cap((256 + tiles_big - 1) / tiles_big)};
  if (tiles_small >= 192)
    return {128, (small_split > 1 && tiles_small < 1024 && nk >= 8) ? cap(small_split) : 1};
  return {128, cap((256 + tiles_small - 1) / tiles_small)};
}

// The K-slices a launch takes when `want` are asked for: whole K-tiles of kt elements per slice,
// and only the slices that have any (so the count can shrink: 9 K-tiles in 4 slices = 3 + 3 + 3)
struct KSlices {
  int k_per_split, splits;
};
inline KSlices k_slices(int K, int kt, int want) {
  const int nkt = K / kt, s = std::max(1, std::min(want, nkt));
  const int kps = (nkt + s - 1) / s * kt;
  return {kps, kps > 0 ? (K + kps - 1) / kps : 1};
}

// Zero-copy k-rows (GemmArgs.qrow): the row table of one K-slice sits in LDS after the staging ring
constexpr int kMaxIdxRows = 8192;
inline bool row_table_fits(int K, int kt, int want_splits) {
  return k_slices(K, kt, want_splits).k_per_split <= kMaxIdxRows;
}

// Capped grid (GM2_OPT_GRID_CAP): the same number of rounds on fewer workgroups, each looping over
// tiles wg, wg + grid, ...; ntiles = 0 when every tile has its own workgroup (no loop)
struct GridCap {
  int grid, ntiles;
};
inline GridCap capped_grid(int tiles, int cus) {
  const int rounds = (tiles + cus - 1) / cus, grid = (tiles + rounds - 1) / rounds;
  return {grid, grid < tiles ? tiles : 0};
}

// ---- split-K slices against the capacity (fp32 elements) of a stream's slab scratch ----
// Into slabs (api.hip gemm_to_slabs: the GEMMs whose consumer sums the slabs itself -- the
// pre-BatchNorm Linears, the heads, the input gradients; plain and bf16x3 alike): slabs of the
// padded rows at the consumer's pitch, the plan's count clamped to what fits; none fitting is an error
inline int64_t slab_elems_padded(int Mp, int64_t ldc) { return (int64_t)Mp * ldc; }
inline int splits_into_slabs(int plan, int64_t slab, int64_t cap) {
  const int S = (int)std::min<int64_t>(plan, cap / std::max<int64_t>(slab, 1));
  if (S < 1) throw std::runtime_error("slab capacity exceeded");
  return S;
}
// Into C (api.hip gemm_to: the weight gradients, summed by k_slab_sum): dense M x N slabs. When the
// plan's slabs do not fit, the plain GEMMs (shrink = false) run one pass straight into C; the bf16x3
// ones (shrink = true: dW9, dWe0) take as many slices as fit. Two behaviours on purpose kept apart:
// DESIGN.md "GEMM launch geometry" has what is known of why
inline int64_t slab_elems_dense(int M, int N) { return ((int64_t)M * N + 3) / 4 * 4; }
inline int splits_into_c(int plan, int64_t slab, int64_t cap, bool shrink) {
  if ((int64_t)plan * slab <= cap) return plan;
  return shrink ? (int)std::max<int64_t>(1, cap / slab) : 1;
}

}  // namespace gm2
