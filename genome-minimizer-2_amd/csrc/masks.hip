// Consumers of the sampled masks, on the packed masks in HBM:
//   * count_essential_genes (utils/extras.py:49-87): per sample, the number of essential genes
//     present, a gene counting when ANY of its column positions is set;
//   * masks_to_gene_lists (explore_data/binary_converter.py:19-76): per sample, the ascending
//     column indices of the set genes (duplicate gene names dropped through a keep mask), as a
//     CSR (row offsets = exclusive scan of row popcounts, then a wave-parallel compaction);
//   * the integer cross products of two sets of rows (no reference kernel: its PCA of the strains,
//     explore_data/data_exploration.py:394-420, unpacks to float64): popcount(a AND b), the Gram
//     matrix of 0/1 rows, and the nearest row by popcount(a XOR b). VALU-bound, LDS-tiled.
//   * genomes per gene (explore_data/data_exploration.py:119-120, `sum(axis=0)` of the 0/1 matrix):
//     the column sums of the bit rows on bit-sliced carry-save counters, every row byte read once.
//   * the genome minimizer's sizes (minimizer/minimizer_2.py:50-101, :273-424): per sample, the gene
//     features it removes from the GenBank record, the bases their union covers and a signature of the
//     merged removed regions (equal signature = the same minimized sequence), from a bit gather per
//     feature and a prefix-max scan over the features sorted by start.
// Mask rows are numpy packbits(bitorder='little') bytes: bit (g & 7) of byte g / 8 = gene g,
// row pitch ld_bits (multiple of 16 bytes), bits beyond G zero. The first two are HBM-bound integer
// work: their kernels stream each mask row once with 16-byte (or 4-byte word) loads.
#include "../../include/gm2.h"
#include "gm2_common.hpp"
#include "gm2_kernels.hpp"

namespace gm2 {

namespace {

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wave per sample row; lane l evaluates groups l, l+64, ...: a group counts when any of its
// positions is set (the reference's `break` after the first present position)
__global__ __launch_bounds__(256) void k_count_groups(const uint8_t* __restrict__ bits, int64_t n, int64_t ldb,
                                                    const int32_t* __restrict__ goff, int ngroups,
                                                    const int32_t* __restrict__ pos, int32_t* __restrict__ counts) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const uint8_t* r = bits + row * ldb;
  int cnt = 0;
  for (int gi = lane; gi < ngroups; gi += 64) {
    int any = 0;
    GM2_DBG(goff[gi] >= 0 && goff[gi] <= goff[gi + 1], kDbgMaskPos);
    for (int k = goff[gi]; k < goff[gi + 1] && !any; ++k) {
      const int p = pos[k];
      GM2_DBG(p >= 0 && (int64_t)(p >> 3) < ldb, kDbgMaskPos);
      any = (r[p >> 3] >> (p & 7)) & 1;
    }
    cnt += any;
  }
  cnt = wave_sum_i(cnt);
  if (lane == 0) counts[row] = cnt;
}

// The same count from whole-row reads: each workgroup first turns the groups into an LDS bit mask of
// the single-position groups (one atomicOr per group; a position already in the mask -- a second
// group on the same gene -- and every multi-position group go to an LDS list instead), then its
// waves stream their rows with 16-byte loads: count = popcount(row AND mask) + the listed groups
// evaluated as above. The same integer as k_count_groups; a row's ~300 scattered byte reads touched
// nearly every line of the row anyway, now one coalesced pass reads it.
constexpr int kCountRowsPerWg = 16;
__global__ __launch_bounds__(256) void k_count_groups_rows(const uint8_t* __restrict__ bits, int64_t n, int64_t ldb,
                                                         const int32_t* __restrict__ goff, int ngroups,
                                                         const int32_t* __restrict__ pos, int32_t* __restrict__ counts,
                                                         int stage) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lmask[];  // [ldb / 4] words, then the list
  const int nw = (int)(ldb / 4);
  int* glist = (int*)(lmask + nw);
  int* gcount = glist + ngroups;
  // (stage: each wave keeps the row it streams in an LDS row buffer [4][ldb], and the listed groups'
  // byte reads go there instead of back to global memory -- they were ~4x the rows' own bytes)
  uint8_t* wrow = (uint8_t*)lmask + ((ldb + (int64_t)(ngroups + 1) * 4 + 15) & ~(int64_t)15) +
                  (int64_t)(threadIdx.x >> 6) * ldb;
  for (int i = threadIdx.x; i < nw; i += 256) lmask[i] = 0u;
  if (threadIdx.x == 0) *gcount = 0;
  __syncthreads();
  for (int g = threadIdx.x; g < ngroups; g += 256) {
    const int k0 = goff[g], k1 = goff[g + 1];
    GM2_DBG(k0 >= 0 && k0 <= k1, kDbgMaskPos);
    if (k1 == k0) continue;  // (an empty group never counts)
    if (k1 - k0 == 1) {
      const int p = pos[k0];
      GM2_DBG(p >= 0 && (int64_t)(p >> 3) < ldb, kDbgMaskPos);
      const uint32_t bit = 1u << (p & 31);
      if (!(atomicOr(&lmask[p >> 5], bit) & bit)) continue;
    }
    glist[atomicAdd(gcount, 1)] = g;
  }
  __syncthreads();
  const int ng = *gcount, lane = threadIdx.x & 63;
  const int64_t r1 = min(n, (int64_t)(blockIdx.x + 1) * kCountRowsPerWg);
  for (int64_t row = (int64_t)blockIdx.x * kCountRowsPerWg + (threadIdx.x >> 6); row < r1; row += 4) {
    const uint8_t* rb = bits + row * ldb;
    const uint4* r = (const uint4*)rb;
    const uint4* m = (const uint4*)lmask;
    int c = 0;
    // (four 16-byte loads per lane in flight before their first use)
    for (int i0 = lane; i0 < nw / 4; i0 += 4 * 64) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = i0 + u * 64 < nw / 4 ? r[i0 + u * 64] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i0 + u * 64 >= nw / 4) break;
        if (stage) ((uint4*)wrow)[i0 + u * 64] = v[u];
        const uint4 k = m[i0 + u * 64];
        c += __builtin_popcount(v[u].x & k.x) + __builtin_popcount(v[u].y & k.y) +
             __builtin_popcount(v[u].z & k.z) + __builtin_popcount(v[u].w & k.w);
      }
    }
    const uint8_t* lb = stage ? wrow : rb;
    if (stage) {  // (this wave's row writes, visible to its own lanes' reads below)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
    for (int j = lane; j < ng; j += 64) {
      const int g = glist[j];
      int any = 0;
      for (int k = goff[g]; k < goff[g + 1] && !any; ++k) {
        const int p = pos[k];
        GM2_DBG(p >= 0 && (int64_t)(p >> 3) < ldb, kDbgMaskPos);
        any = (lb[p >> 3] >> (p & 7)) & 1;
      }
      c += any;
    }
    if (stage) __builtin_amdgcn_wave_barrier();  // (the next row overwrites the buffer after these reads)
    c = wave_sum_i(c);
    if (lane == 0) counts[row] = c;
  }
}

// popcount of each row (AND keep mask) -> out[row]; one wave per row, 16-byte loads
__global__ __launch_bounds__(256) void k_row_popcount(const uint8_t* __restrict__ bits, int64_t n, int64_t ldb,
                                                    const uint8_t* __restrict__ keep, int64_t* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const uint4* r = (const uint4*)(bits + row * ldb);
  const uint4* kp = (const uint4*)keep;
  int c = 0;
  for (int64_t i = lane; i < ldb / 16; i += 64) {
    uint4 v = r[i];
    if (kp) {
      const uint4 k = kp[i];
      v.x &= k.x; v.y &= k.y; v.z &= k.z; v.w &= k.w;
    }
    c += __builtin_popcount(v.x) + __builtin_popcount(v.y) + __builtin_popcount(v.z) + __builtin_popcount(v.w);
  }
  c = wave_sum_i(c);
  if (lane == 0) out[row] = c;
}

// in-place inclusive scan of a[0..n) (int64), one workgroup of 1024 threads: per-thread chunk sums,
// an LDS scan of the 1024 sums, then each chunk rewritten with its offset
__global__ __launch_bounds__(1024) void k_scan_inclusive(int64_t* __restrict__ a, int64_t n) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const int64_t chunk = (n + 1023) / 1024;
  const int64_t lo = t * chunk, hi = min(n, lo + chunk);
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += a[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const int64_t v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = t ? part[t - 1] : 0;
  for (int64_t i = lo; i < hi; ++i) {
    run += a[i];
    a[i] = run;
  }
}

// set-bit column indices of each row in ascending order at out[off[row] ...]: one wave per row,
// 64 words per pass (lane l holds word base + l), exclusive wave scan of the word popcounts
__global__ __launch_bounds__(256) void k_compact(const uint8_t* __restrict__ bits, int64_t n, int64_t ldb,
                                               const uint8_t* __restrict__ keep, const int64_t* __restrict__ off,
                                               int32_t* __restrict__ idx) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const uint32_t* r = (const uint32_t*)(bits + row * ldb);
  const uint32_t* kp = (const uint32_t*)keep;
  int64_t out = off[row];
  const int64_t nw = ldb / 4;
  for (int64_t base = 0; base < nw; base += 64) {
    const int64_t wi = base + lane;
    uint32_t w = wi < nw ? r[wi] : 0u;
    if (kp && wi < nw) w &= kp[wi];
    const int c = __builtin_popcount(w);
    int pre = c;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(pre, o, 64);
      if (lane >= o) pre += v;
    }
    const int tot = __shfl(pre, 63, 64);
    int64_t dst = out + pre - c;
    while (w) {
      const int b = __builtin_ctz(w);
      GM2_DBG(dst >= off[row] && dst < off[row + 1], kDbgCompact);
      idx[dst++] = (int32_t)(wi * 32 + b);
      w &= w - 1;
    }
    out += tot;
  }
}

// ---- bit-row cross products: out[i][j] = popcount(a_i OP b_j), OP = AND (co-occurrence, the Gram
// matrix of 0/1 rows) or XOR (Hamming distance) ----
// A workgroup of 256 lanes owns a 64 x 64 tile of (A row, B row) pairs and walks the rows' bytes in
// chunks of kBgChunk: both 64-row tiles of the chunk are staged in LDS with 16-byte global loads (the
// next chunk's loads are in flight while this one is consumed), rows beyond na / nb and bytes beyond
// the row's kb zero-filled there. Lane (ty = t / 16, tx = t % 16) accumulates the 4 x 4 block of pairs
// (A rows ty + 16 r, B rows tx + 16 c): per 16 bytes of the rows 8 ds_read_b128 feed 64
// (v_and | v_xor) + v_bcnt_u32_b32 pairs, i.e. 16 x 128 gene pairs. LDS rows are pitched kBgChunk + 16
// bytes = an odd number of 16-byte slots, so the 16 B rows a ds_read_b128 lane group reads sit on 16
// different slots of the 256-byte bank row, and its 2 A rows (every other lane a broadcast) on two.
constexpr int kBgTile = 64;
constexpr int kBgChunk = 128;             // bytes of each row per LDS stage (1024 genes)
constexpr int kBgPitch = kBgChunk + 16;   // 9 slots of 16 bytes
constexpr int kBgPieces = kBgTile * (kBgChunk / 16) / 256;  // 16-byte pieces per lane per operand

struct BitTile {
  uint4 a[kBgPieces], b[kBgPieces];
};

// the chunk at byte k0 of both tiles -> registers (zero beyond the rows / the row bytes)
__device__ __forceinline__ void bg_load(BitTile& t, const uint8_t* __restrict__ A, int64_t na, int64_t lda, int64_t i0,
                                        const uint8_t* __restrict__ B, int64_t nb, int64_t ldb, int64_t j0,
                                        int64_t k0, int64_t kb) {
#pragma unroll
  for (int p = 0; p < kBgPieces; ++p) {
    const int piece = threadIdx.x + p * 256, row = piece >> 3;
    const int64_t k = k0 + (piece & 7) * 16;
    t.a[p] = t.b[p] = make_uint4(0u, 0u, 0u, 0u);
    if (i0 + row < na && k < kb) t.a[p] = *(const uint4*)(A + (i0 + row) * lda + k);
    if (j0 + row < nb && k < kb) t.b[p] = *(const uint4*)(B + (j0 + row) * ldb + k);
  }
}

__device__ __forceinline__ void bg_stage(const BitTile& t, uint8_t* la, uint8_t* lb) {
#pragma unroll
  for (int p = 0; p < kBgPieces; ++p) {
    const int piece = threadIdx.x + p * 256, o = (piece >> 3) * kBgPitch + (piece & 7) * 16;
    *(uint4*)(la + o) = t.a[p];
    *(uint4*)(lb + o) = t.b[p];
  }
}

template <bool kXor>
__device__ __forceinline__ int bg_pop(const uint4& x, const uint4& y, int acc) {
  if (kXor) {
    acc += __builtin_popcount(x.x ^ y.x);
    acc += __builtin_popcount(x.y ^ y.y);
    acc += __builtin_popcount(x.z ^ y.z);
    acc += __builtin_popcount(x.w ^ y.w);
  } else {
    acc += __builtin_popcount(x.x & y.x);
    acc += __builtin_popcount(x.y & y.y);
    acc += __builtin_popcount(x.z & y.z);
    acc += __builtin_popcount(x.w & y.w);
  }
  return acc;
}

// acc[r][c] = popcount(A[i0 + ty + 16 r] OP B[j0 + tx + 16 c]) over the rows' first kb bytes
template <bool kXor>
__device__ __forceinline__ void bg_tile(const uint8_t* __restrict__ A, int64_t na, int64_t lda, int64_t i0,
                                        const uint8_t* __restrict__ B, int64_t nb, int64_t ldb, int64_t j0, int64_t kb,
                                        int (&acc)[4][4]) {
  __shared__ __attribute__((aligned(16))) uint8_t la[kBgTile * kBgPitch];
  __shared__ __attribute__((aligned(16))) uint8_t lb[kBgTile * kBgPitch];
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0;
  BitTile t;
  bg_load(t, A, na, lda, i0, B, nb, ldb, j0, 0, kb);
  for (int64_t k0 = 0; k0 < kb; k0 += kBgChunk) {
    __syncthreads();  // (the previous chunk's reads are done)
    bg_stage(t, la, lb);
    __syncthreads();
    if (k0 + kBgChunk < kb) bg_load(t, A, na, lda, i0, B, nb, ldb, j0, k0 + kBgChunk, kb);
#pragma unroll
    for (int s = 0; s < kBgChunk / 16; ++s) {
      uint4 x[4], y[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) x[r] = *(const uint4*)(la + (ty + 16 * r) * kBgPitch + s * 16);
#pragma unroll
      for (int c = 0; c < 4; ++c) y[c] = *(const uint4*)(lb + (tx + 16 * c) * kBgPitch + s * 16);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = bg_pop<kXor>(x[r], y[c], acc[r][c]);
    }
  }
}

// tiles in a 1-D grid, B tiles fastest: neighbouring workgroups share their A tile and walk B, which
// (7,512 F4 rows = 52 MB) stays in the last-level cache
__global__ __launch_bounds__(256) void k_bit_cooccur(const uint8_t* __restrict__ A, int64_t na, int64_t lda,
                                                   const uint8_t* __restrict__ B, int64_t nb, int64_t ldb, int64_t kb,
                                                   int32_t* __restrict__ out, int64_t ldo, int tiles_b) {
  const int64_t i0 = (int64_t)(blockIdx.x / tiles_b) * kBgTile, j0 = (int64_t)(blockIdx.x % tiles_b) * kBgTile;
  int acc[4][4];
  bg_tile<false>(A, na, lda, i0, B, nb, ldb, j0, kb, acc);
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t i = i0 + ty + 16 * r;
    if (i >= na) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t j = j0 + tx + 16 * c;
      if (j >= nb) continue;
      GM2_DBG(i >= 0 && j >= 0 && j < ldo && i * ldo + j < na * ldo, kDbgBitRows);
      out[i * ldo + j] = acc[r][c];
    }
  }
}

// best[i] = min over the tile's reference rows j of (distance << 32 | j), merged into global memory
// with a 64-bit atomic min: the keys are non-negative and unique per (distance, j), so the minimum
// is the nearest row, the lowest index among ties, whatever order the tiles arrive in
__global__ __launch_bounds__(256) void k_bit_nearest(const uint8_t* __restrict__ Q, int64_t nq, int64_t ldq,
                                                   const uint8_t* __restrict__ R, int64_t nr, int64_t ldr, int64_t kb,
                                                   unsigned long long* __restrict__ best, int tiles_r) {
  const int64_t i0 = (int64_t)(blockIdx.x / tiles_r) * kBgTile, j0 = (int64_t)(blockIdx.x % tiles_r) * kBgTile;
  int acc[4][4];
  bg_tile<true>(Q, nq, ldq, i0, R, nr, ldr, j0, kb, acc);
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    unsigned long long key = ~0ull >> 1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t j = j0 + tx + 16 * c;
      const unsigned long long k = ((unsigned long long)(unsigned)acc[r][c] << 32) | (unsigned long long)j;
      if (j < nr && k < key) key = k;
    }
    // (the 16 lanes of one ty are 16 neighbouring lanes of a wave)
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
      const unsigned long long v = __shfl_xor(key, o, 64);
      key = v < key ? v : key;
    }
    const int64_t i = i0 + ty + 16 * r;
    if (tx == 0 && i < nq) {
      GM2_DBG(i >= 0 && (key & 0xffffffffull) < (unsigned long long)nr, kDbgBitRows);
      atomicMin(&best[i], key);
    }
  }
}

__global__ __launch_bounds__(256) void k_fill_u64(unsigned long long* __restrict__ p, int64_t n, unsigned long long v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

// ---- per-gene counts: counts[g] += number of the selected rows with gene g set (the column sums of
// the bit matrix, a positional popcount) ----
// A workgroup of 4 waves owns a column chunk of 64 x 16 bytes (8,192 genes) and a slab of the selected
// rows; lane l of every wave owns the 16-byte piece 64 chunk + l of each row (4 words, 128 genes), so
// one wave-instruction loads 1 KiB of one row. Wave w takes the slab's 8-row blocks w, w + 4, ...:
// the 8 pieces of a block are loaded together, the next block's before this one is added (two
// register buffers: 8 KiB in flight per wave under the arithmetic, 128 KiB per CU at 4 workgroups),
// then added into 8 bit-sliced planes per word (bit b of p[k] = bit k of the running count of gene
// 32 word + b; 126 VGPRs, no scratch): a carry-save tree reduces the 8 rows into
// planes 0-2 and one carry word of weight 8 (7 adders of 5 operations), which ripples through planes
// 3-7 (10 operations): 45 VALU operations per 8 x 32 bits. A block adds at most 8 to a plane counter,
// so after kGcFlushBlocks = 31 blocks (P = 248 rows of the wave, <= 255) the planes are spilled into
// the workgroup's LDS counters (ds_add_u32, [gene of the lane][lane] pitched 65: the lanes of one add
// and of one read below on 64 banks) and cleared. At the end every non-zero LDS sum of a gene < G goes
// to counts with one 64-bit global atomic add: integer adds commute, so the result is exact whatever
// order the slabs arrive in.
constexpr int kGcPieces = 64;         // 16-byte pieces of a row per workgroup (one per lane)
constexpr int kGcGenes = 128;         // genes of a piece
constexpr int kGcBlock = 8;           // rows per carry-save block
constexpr int kGcWaves = 4;
constexpr int kGcFlushBlocks = 31;    // blocks between two spills: 31 * 8 = 248 <= 2^8 - 1
constexpr int kGcSlabRows = 1024;     // fewest rows of a slab (a multiple of kGcWaves * kGcBlock)
constexpr int kGcTargetWgs = 1024;    // workgroups of a large call: 256 CUs x 4 resident (33 KB of LDS
                                      // each); 2,048 measured 3 % slower
constexpr int kGcPitch = kGcPieces + 1;

// (h, l) = carry and sum of a + b + c, bit-sliced
#define GM2_CSA(h, l, a, b, c)               \
  do {                                       \
    const uint32_t u_ = (a) ^ (b), c_ = (c); \
    (h) = ((a) & (b)) | (u_ & c_);           \
    (l) = u_ ^ c_;                           \
  } while (0)

// the 8 pieces of the block at list position i (rows beyond r1 and lanes beyond the row: zero; their
// loads go to the last row / piece instead of branching)
template <bool kIdx>
__device__ __forceinline__ void gc_load(uint4 (&x)[kGcBlock], const uint4* __restrict__ col, int64_t ld16,
                                        const int32_t* __restrict__ rows, int64_t n_rows, int64_t i, int64_t r1,
                                        bool active) {
#pragma unroll
  for (int u = 0; u < kGcBlock; ++u) {
    int64_t src = min(i + u, r1 - 1);
    if (kIdx) {
      src = rows[src];
      GM2_DBG(src >= 0 && src < n_rows, kDbgGeneRows);
    }
    x[u] = col[src * ld16];
  }
#pragma unroll
  for (int u = 0; u < kGcBlock; ++u)
    if (!(active && i + u < r1)) x[u] = make_uint4(0u, 0u, 0u, 0u);
}

// 8 rows of one word column into its planes
__device__ __forceinline__ void gc_add(uint32_t (&p)[8], uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3,
                                       uint32_t x4, uint32_t x5, uint32_t x6, uint32_t x7) {
  uint32_t t2a, t2b, t4a, t4b, c8;
  GM2_CSA(t2a, p[0], p[0], x0, x1);
  GM2_CSA(t2b, p[0], p[0], x2, x3);
  GM2_CSA(t4a, p[1], p[1], t2a, t2b);
  GM2_CSA(t2a, p[0], p[0], x4, x5);
  GM2_CSA(t2b, p[0], p[0], x6, x7);
  GM2_CSA(t4b, p[1], p[1], t2a, t2b);
  GM2_CSA(c8, p[2], p[2], t4a, t4b);
#pragma unroll
  for (int k = 3; k < 8; ++k) {
    const uint32_t c = p[k] & c8;
    p[k] ^= c8;
    c8 = c;
  }
}

struct GcPlanes {
  uint32_t x[8], y[8], z[8], w[8];  // the planes of the lane's 4 words
};

// the planes' counts into the LDS counters of the lane's 128 genes; planes cleared
__device__ __forceinline__ void gc_flush_word(uint32_t (&p)[8], unsigned* __restrict__ l) {
#pragma unroll
  for (int b = 0; b < 32; ++b) {
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += ((p[k] >> b) & 1u) << k;
    atomicAdd(&l[b * kGcPitch], v);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = 0u;
}
__device__ __forceinline__ void gc_flush(GcPlanes& pl, unsigned* __restrict__ lsum, int lane) {
  gc_flush_word(pl.x, lsum + lane);
  gc_flush_word(pl.y, lsum + 32 * kGcPitch + lane);
  gc_flush_word(pl.z, lsum + 64 * kGcPitch + lane);
  gc_flush_word(pl.w, lsum + 96 * kGcPitch + lane);
}

template <bool kIdx>
__global__ __launch_bounds__(256) void k_gene_counts(const uint8_t* __restrict__ bits, int64_t n_rows, int64_t ldb, int n16,
                                                   int64_t G, const int32_t* __restrict__ rows, int64_t n,
                                                   int64_t slab_rows, int nc, unsigned long long* __restrict__ counts) {
  __shared__ __attribute__((aligned(16))) unsigned lsum[kGcGenes * kGcPitch];
  const int chunk = blockIdx.x % nc;  // chunks fastest: neighbouring workgroups read the same rows
  const int64_t slab = blockIdx.x / nc;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int piece = chunk * kGcPieces + lane;
  const bool active = piece < n16;  // (pieces beyond roundup(G, 128) / 128 are never read)
  const uint4* col = (const uint4*)bits + min(piece, n16 - 1);
  const int64_t ld16 = ldb / 16;
  const int64_t r1 = min(n, (slab + 1) * slab_rows);
  for (int i = threadIdx.x; i < kGcGenes * kGcPitch / 4; i += 256) ((uint4*)lsum)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  GcPlanes pl;
#pragma unroll
  for (int k = 0; k < 8; ++k) pl.x[k] = pl.y[k] = pl.z[k] = pl.w[k] = 0u;
  int blocks = 0;
  auto add = [&](const uint4(&x)[kGcBlock]) __attribute__((always_inline)) {
    gc_add(pl.x, x[0].x, x[1].x, x[2].x, x[3].x, x[4].x, x[5].x, x[6].x, x[7].x);
    gc_add(pl.y, x[0].y, x[1].y, x[2].y, x[3].y, x[4].y, x[5].y, x[6].y, x[7].y);
    gc_add(pl.z, x[0].z, x[1].z, x[2].z, x[3].z, x[4].z, x[5].z, x[6].z, x[7].z);
    gc_add(pl.w, x[0].w, x[1].w, x[2].w, x[3].w, x[4].w, x[5].w, x[6].w, x[7].w);
    if (++blocks == kGcFlushBlocks) {
      gc_flush(pl, lsum, lane);
      blocks = 0;
    }
  };

  constexpr int kStep = kGcWaves * kGcBlock;
  int64_t i = slab * slab_rows + (int64_t)wave * kGcBlock;
  if (i < r1) {
    uint4 xa[kGcBlock], xb[kGcBlock];
    gc_load<kIdx>(xa, col, ld16, rows, n_rows, i, r1, active);
    while (true) {  // (a load beyond the slab reads its last row again and keeps zeros)
      gc_load<kIdx>(xb, col, ld16, rows, n_rows, i + kStep, r1, active);
      add(xa);
      if ((i += kStep) >= r1) break;
      gc_load<kIdx>(xa, col, ld16, rows, n_rows, i + kStep, r1, active);
      add(xb);
      if ((i += kStep) >= r1) break;
    }
    gc_flush(pl, lsum, lane);
  }
  __syncthreads();
#pragma unroll 4
  for (int k = 0; k < kGcGenes * kGcPieces / 256; ++k) {
    const int gl = threadIdx.x + 256 * k;  // gene 128 (gl >> 7) + (gl & 127) of the chunk
    const unsigned v = lsum[(gl & (kGcGenes - 1)) * kGcPitch + (gl >> 7)];
    const int64_t g = (int64_t)chunk * (kGcGenes * kGcPieces) + gl;
    if (g < G && v) atomicAdd(&counts[g], (unsigned long long)v);
  }
}
#undef GM2_CSA

// ---- bit transpose: out row g, bit i = bits row i, bit g (the same packed layout on both sides) ----
// A workgroup of 512 lanes owns a tile of 1,024 source rows x 512 genes: 64 bytes of each source row in,
// one whole 128-byte line of each of 512 output rows out (the other way round, 512 rows x 1,024 genes
// with whole lines in and half lines out, measured 1.3x slower). Lane (rb = t / 16, j = t % 16) owns the
// 32 x 32 bit block of rows 32 rb .. 32 rb + 31 and gene word j: its 32 global loads (one word each;
// the 16 lanes of one rb read 64 contiguous bytes of a row, a wave 4 rows per load) are all in
// flight together. In a tile that reaches past the n rows or past roundup(G, 128) / 32 words the loads
// go to the last valid row / word instead and are zeroed in registers, so no lane branches; an interior
// tile (a test uniform over the workgroup) skips the clamps. The block is transposed in registers by
// the 5 block-swap stages of the recursive 32 x 32 transpose (16 swaps of 6 operations each per
// stage: 480 VALU operations per 1,024 bits and lane, no cross-lane traffic), after which register b
// holds the 4 output bytes (rows 32 rb ..) of gene 32 j + b.
// These go through an LDS tile [512 genes][32 words] (64 KB, two workgroups per CU) so that the
// global stores are whole lines: the word of (gene g, row block rb) sits at column
// (rb + 2 (g / 32) + g % 4) % 32 of row g. The pitch is a whole 128-byte bank row (ds_write_b32 and
// ds_read_b32 bank = word address mod 32 = the column, conflicts counted per 32-lane half):
//   * a store's half holds 2 row blocks (rb even, rb + 1) x 16 words j of one register b: columns
//     rb' + 2 j + const, 32 different banks;
//   * a read's half holds the 8 pieces q of 4 neighbouring genes (g % 4 = 0..3, one g / 32) and reads
//     word c of each piece: columns 4 q + g % 4 + const, 32 different banks.
// Each lane then gathers 8 16-byte pieces (4 ds_read_b32 each) and stores them with 16-byte stores:
// 8 neighbouring lanes write one 128-byte line of one gene row.
constexpr int kTrThreads = 512;           // one 32 x 32 block per lane
constexpr int kTrWords = 16;              // 32-gene words of a tile (64 bytes of a source row)
constexpr int kTrRb = kTrThreads / kTrWords;  // row blocks of a tile = words of an LDS row
constexpr int kTrRows = 32 * kTrRb;       // source rows of a tile (128 bytes of an output row)
constexpr int kTrGenes = 32 * kTrWords;
constexpr int kTrPc = kTrRb / 4;          // 16-byte pieces of an output row per tile

static_assert(kTrRb == 32 && kTrWords == 16, "tr_col's bank analysis is for LDS rows of 32 words, 16 words j per row block");
__device__ __forceinline__ int tr_col(int g, int rb) { return (rb + 2 * (g >> 5) + (g & 3)) & 31; }

// a[i] bit c <-> a[c] bit i: at scale j the blocks (rows without bit j, columns with it) and (rows
// with bit j, columns without it) change places
__device__ __forceinline__ void tr_32x32(uint32_t (&a)[32]) {
#pragma unroll
  for (int j = 16; j; j >>= 1) {
    const uint32_t m = 0xffffffffu / ((1u << j) + 1u);  // the columns without bit j
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      if (k & j) continue;
      const uint32_t t = ((a[k] >> j) ^ a[k + j]) & m;
      a[k + j] ^= t;
      a[k] ^= t << j;
    }
  }
}

// the 32 words of the lane's block: rows row .. row + 31 of word w. kEdge: a tile that reaches past the
// n rows or the kw readable words of a row (loads clamped to the last valid row / word, then zeroed);
// else the addresses are one lane base plus a uniform multiple of the pitch
template <bool kEdge>
__device__ __forceinline__ void tr_load(uint32_t (&a)[32], const uint8_t* __restrict__ bits, int64_t n, int64_t ldb,
                                        int64_t kw, int64_t w, int64_t row) {
  if (kEdge) {
    const uint8_t* src = bits + min(w, kw - 1) * 4;
#pragma unroll
    for (int i = 0; i < 32; ++i) a[i] = *(const uint32_t*)(src + min(row + i, n - 1) * ldb);
#pragma unroll
    for (int i = 0; i < 32; ++i)
      if (!(w < kw && row + i < n)) a[i] = 0u;
  } else {
    const uint8_t* src = bits + row * ldb + w * 4;
#pragma unroll
    for (int i = 0; i < 32; ++i) a[i] = *(const uint32_t*)(src + i * ldb);
  }
}

// Tiles in a 1-D grid, in bands of kTrBand gene tiles: inside a band the gene tiles run fastest, then
// the row tiles, so the few hundred workgroups in flight together read kTrBand * kTrWords * 4
// contiguous bytes of each of their rows and write neighbouring lines of the same gene rows (gene tiles
// fastest over the whole width had every 128-byte store of a moment on a line of its own row,
// roundup(n, 128) / 8 bytes from the next: 7.4 ms against 4.0 ms at 1e6 x 55,039; bands of 8 and of 32
// measured 3-6 % slower than 16)
constexpr int kTrBand = 16;
__global__ __launch_bounds__(kTrThreads) void k_bit_transpose(const uint8_t* __restrict__ bits, int64_t n, int64_t ldb,
                                                            int64_t kw, int64_t G, uint8_t* __restrict__ out,
                                                            int64_t ldo, int64_t ob, int tiles_g, int tiles_r) {
  __shared__ __attribute__((aligned(16))) uint32_t lt[kTrGenes * kTrRb];
  const int band = blockIdx.x / (kTrBand * tiles_r), in_band = blockIdx.x - band * (kTrBand * tiles_r);
  const int band_tiles = min(kTrBand, tiles_g - band * kTrBand);  // (the last band may be narrower)
  const int64_t r0 = (int64_t)(in_band / band_tiles) * kTrRows;
  const int64_t w0 = (int64_t)(band * kTrBand + in_band % band_tiles) * kTrWords;
  const int j = threadIdx.x & (kTrWords - 1), rb = threadIdx.x / kTrWords;
  uint32_t a[32];
  if (r0 + kTrRows <= n && w0 + kTrWords <= kw)  // (uniform over the workgroup)
    tr_load<false>(a, bits, n, ldb, kw, w0 + j, r0 + 32 * rb);
  else
    tr_load<true>(a, bits, n, ldb, kw, w0 + j, r0 + 32 * rb);
  tr_32x32(a);
#pragma unroll
  for (int b = 0; b < 32; ++b) lt[(32 * j + b) * kTrRb + tr_col(32 * j + b, rb)] = a[b];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kTrGenes * kTrPc / kTrThreads; ++k) {
    const int p = threadIdx.x + kTrThreads * k, g = p / kTrPc, q = p % kTrPc;
    const uint32_t* lr = lt + g * kTrRb;
    const uint4 v = make_uint4(lr[tr_col(g, 4 * q)], lr[tr_col(g, 4 * q + 1)], lr[tr_col(g, 4 * q + 2)],
                               lr[tr_col(g, 4 * q + 3)]);
    const int64_t gene = w0 * 32 + g, byte = r0 / 8 + 16 * q;
    if (gene < G && byte < ob) {  // (ob: the bytes of an output row that are written, a multiple of 16)
      GM2_DBG(gene >= 0 && gene < G && byte >= 0 && byte + 16 <= (n + 127) / 128 * 16 && byte + 16 <= ldo, kDbgTranspose);
      *(uint4*)(out + gene * ldo + byte) = v;
    }
  }
}

// ---- minimized genome sizes: what GenomeMinimiser (minimizer/minimizer_2.py:50-101) would cut from the
// GenBank record for each sampled row, without the sequence ----
// The record's gene features arrive sorted by start as three int32 tables: col (>= 0: the feature is
// kept iff that bit of the row is set; -1: always removed; -2: always kept), start and end ([start, end)
// clipped to the record). Per row: the number of removed features, the length of the union of the
// removed non-empty intervals, and a 64-bit signature of the merged intervals (the sum over them of
// mix(2 start) + mix(2 end + 1), mix = the splitmix64 finalizer; integer adds commute, so the order of
// the reduction does not matter). One wave per row, kMsRowsPerWg rows per workgroup; the wave first
// copies its row into LDS (16-byte loads, every row byte read once) when four rows fit in 64 KB, and the
// per-feature bit gathers go there. The features are walked in chunks of 64, feature = chunk * 64 + lane
// (coalesced table loads, the next chunk's in flight under this one's scan; the tables stay in L2). With
// the starts ascending, the merged intervals follow from a running maximum: cover = the largest end of the
// removed non-empty features before this one = max(wave-uniform carry of the earlier chunks, exclusive
// prefix max over the lanes). The feature adds max(0, end - max(start, cover)) bases; it opens a new
// interval iff start > cover (touching intervals merge), and then cover, if any, closed the one before;
// the last interval's end is the carry after the last chunk.
constexpr int kMsRowsPerWg = 16;

__device__ __forceinline__ unsigned long long ms_mix(unsigned long long z) {
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// inclusive prefix max over the wave's 64 lanes of values >= -1 (the identity), on the DPP lane routes:
// shifts by 1, 2, 4, 8 inside each row of 16 lanes (a lane without a source keeps the identity), then
// lane 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3. Six full-rate VALU pairs; the
// same scan with __shfl_up is six ds_bpermute round trips through the LDS crossbar, each waited for.
__device__ __forceinline__ int wave_scan_max(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(-1, v, 0x111, 0xf, 0xf, false));  // row_shr:1
  v = max(v, __builtin_amdgcn_update_dpp(-1, v, 0x112, 0xf, 0xf, false));  // row_shr:2
  v = max(v, __builtin_amdgcn_update_dpp(-1, v, 0x114, 0xf, 0xf, false));  // row_shr:4
  v = max(v, __builtin_amdgcn_update_dpp(-1, v, 0x118, 0xf, 0xf, false));  // row_shr:8
  v = max(v, __builtin_amdgcn_update_dpp(-1, v, 0x142, 0xa, 0xf, false));  // row_bcast:15 -> rows 1, 3
  v = max(v, __builtin_amdgcn_update_dpp(-1, v, 0x143, 0xc, 0xf, false));  // row_bcast:31 -> rows 2, 3
  return v;
}

template <bool kStage>
__global__ __launch_bounds__(256) void k_minimized_stats(const uint8_t* __restrict__ bits, int64_t n, int64_t ldb, int kb16,
                                                       int G, const int32_t* __restrict__ fcol,
                                                       const int32_t* __restrict__ fstart,
                                                       const int32_t* __restrict__ fend, int F,
                                                       int64_t* __restrict__ removed_bp, int32_t* __restrict__ genes_removed,
                                                       unsigned long long* __restrict__ signature) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ms_rows[];  // kStage: [4 waves][kb16 * 16 bytes]
  const int lane = threadIdx.x & 63;
  uint8_t* wrow = ms_rows + (size_t)(threadIdx.x >> 6) * kb16 * 16;
  const int64_t r1 = min(n, (int64_t)(blockIdx.x + 1) * kMsRowsPerWg);
  for (int64_t row = (int64_t)blockIdx.x * kMsRowsPerWg + (threadIdx.x >> 6); row < r1; row += 4) {
    const uint8_t* rb = bits + row * ldb;
    if (kStage) {
      for (int i = lane; i < kb16; i += 64) ((uint4*)wrow)[i] = ((const uint4*)rb)[i];
      // (this wave's row writes, visible to its own lanes' reads below)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
    int carry = -1, gone = 0;  // carry: the largest removed non-empty end of the chunks so far (uniform)
    unsigned long long bp = 0ull, sig = 0ull;
    // (lanes beyond F hold an always-kept feature)
    int c = -2, s = 0, e = 0;
    if (lane < F) c = fcol[lane], s = fstart[lane], e = fend[lane];
    for (int64_t f0 = 0; f0 < F; f0 += 64) {
      int cn = -2, sn = 0, en = 0;
      if (f0 + 64 + lane < F) cn = fcol[f0 + 64 + lane], sn = fstart[f0 + 64 + lane], en = fend[f0 + 64 + lane];
      GM2_DBG(c >= -2 && c < G && (int64_t)(c >> 3) < ldb, kDbgMaskPos);
      bool kept = c == -2;
      if (c >= 0 && c < G) {  // (a column outside the row is never read: the feature counts as removed)
        const int byte = kStage ? wrow[c >> 3] : rb[c >> 3];
        kept = (byte >> (c & 7)) & 1;
      }
      const bool cut = !kept && e > s;  // a removed feature that covers bases
      gone += !kept;
      const int incl = wave_scan_max(cut ? e : -1);
      // (wave_shr:1: the lane before's inclusive max, -1 in lane 0)
      const int cover = max(carry, __builtin_amdgcn_update_dpp(-1, incl, 0x138, 0xf, 0xf, false));
      carry = max(carry, __builtin_amdgcn_readlane(incl, 63));
      if (cut) {
        bp += (unsigned long long)max(0, e - max(s, cover));
        if (s > cover) {
          sig += ms_mix(2ull * (unsigned long long)(unsigned)s);
          if (cover >= 0) sig += ms_mix(2ull * (unsigned long long)(unsigned)cover + 1ull);
        }
      }
      c = cn, s = sn, e = en;
    }
    if (lane == 0 && carry >= 0) sig += ms_mix(2ull * (unsigned long long)(unsigned)carry + 1ull);
    if (kStage) __builtin_amdgcn_wave_barrier();  // (the next row overwrites the buffer after these reads)
    bp = wave_sum_u64(bp);
    sig = wave_sum_u64(sig);
    gone = wave_sum_i(gone);
    if (lane == 0) {
      removed_bp[row] = (int64_t)bp;
      genes_removed[row] = gone;
      signature[row] = sig;
    }
  }
}

// 1-D grid of ta x tb tiles
unsigned bit_grid(int64_t ra, int64_t rb, int* tiles_b) {
  const int64_t ta = (ra + kBgTile - 1) / kBgTile, tb = (rb + kBgTile - 1) / kBgTile;
  if (tb > 0x7fffffff || ta * tb > 0x7fffffff)
    throw Gm2Error("bit rows: %lld x %lld rows are more tiles than one launch holds", (long long)ra, (long long)rb);
  *tiles_b = (int)tb;
  return (unsigned)(ta * tb);
}
}  // namespace

void launch_bit_cooccur(const uint8_t* a, int64_t na, int64_t lda, const uint8_t* b, int64_t nb, int64_t ldb, int64_t G,
                        int32_t* out, int64_t ldo, hipStream_t s) {
  if (na <= 0 || nb <= 0) return;
  int tb;
  const unsigned grid = bit_grid(na, nb, &tb);
  const int64_t kb = (G + 127) / 128 * 16;
  hipLaunchKernelGGL(k_bit_cooccur, dim3(grid), dim3(256), 0, s, a, na, lda, b, nb, ldb, kb, out, ldo, tb);
  GM2_CHECK_LAUNCH();
}

void launch_bit_nearest(const uint8_t* q, int64_t nq, int64_t ldq, const uint8_t* ref, int64_t nr, int64_t ldr, int64_t G,
                        int64_t* best, hipStream_t s) {
  if (nq <= 0) return;
  int tr;
  const unsigned grid = bit_grid(nq, nr, &tr);
  // the identity of the min: all ones in the low 63 bits
  hipLaunchKernelGGL(k_fill_u64, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (unsigned long long*)best, nq,
                     ~0ull >> 1);
  GM2_CHECK_LAUNCH();
  const int64_t kb = (G + 127) / 128 * 16;
  hipLaunchKernelGGL(k_bit_nearest, dim3(grid), dim3(256), 0, s, q, nq, ldq, ref, nr, ldr, kb,
                     (unsigned long long*)best, tr);
  GM2_CHECK_LAUNCH();
}

void launch_gene_counts(const uint8_t* bits, int64_t n_rows, int64_t ldb, int64_t G, const int32_t* rows, int64_t n,
                        int64_t* counts, hipStream_t s) {
  if (n <= 0) return;
  // nc column chunks x enough row slabs for kGcTargetWgs workgroups, a slab no shorter than
  // kGcSlabRows: at most 8,192 atomics (64 KB) per workgroup against >= 1 MB of rows read
  const int64_t nw = (G + 127) / 128, nc = (nw + kGcPieces - 1) / kGcPieces;
  const int64_t slabs = std::max<int64_t>(1, std::min<int64_t>(kGcTargetWgs / nc, (n + kGcSlabRows - 1) / kGcSlabRows));
  const int64_t step = kGcWaves * kGcBlock;
  const int64_t slab_rows = ((n + slabs - 1) / slabs + step - 1) / step * step;
  const int64_t used = (n + slab_rows - 1) / slab_rows;
  if (slab_rows > 0x7fffffff || used * nc > 0x7fffffff)
    throw Gm2Error("mask_gene_counts: %lld rows x %lld genes are more than one launch holds", (long long)n, (long long)G);
  const dim3 grid((unsigned)(used * nc));
  if (rows)
    hipLaunchKernelGGL(k_gene_counts<true>, grid, dim3(256), 0, s, bits, n_rows, ldb, (int)nw, G, rows, n, slab_rows,
                       (int)nc, (unsigned long long*)counts);
  else
    hipLaunchKernelGGL(k_gene_counts<false>, grid, dim3(256), 0, s, bits, n_rows, ldb, (int)nw, G, rows, n, slab_rows,
                       (int)nc, (unsigned long long*)counts);
  GM2_CHECK_LAUNCH();
}

void launch_bit_transpose(const uint8_t* bits, int64_t n, int64_t ldb, int64_t G, uint8_t* out, int64_t ldo,
                          hipStream_t s) {
  if (n <= 0) return;
  const int64_t tr = (n + kTrRows - 1) / kTrRows, tg = (G + kTrGenes - 1) / kTrGenes;
  if (tr * tg > 0x7fffffff)
    throw Gm2Error("mask_transpose: %lld rows x %lld genes are more tiles than one launch holds", (long long)n,
                   (long long)G);
  const int64_t kw = (G + 127) / 128 * 4, ob = (n + 127) / 128 * 16;
  hipLaunchKernelGGL(k_bit_transpose, dim3((unsigned)(tr * tg)), dim3(kTrThreads), 0, s, bits, n, ldb, kw, G, out, ldo,
                     ob, (int)tg, (int)tr);
  GM2_CHECK_LAUNCH();
}

void launch_minimized_stats(const uint8_t* bits, int64_t n, int64_t ldb, int64_t G, const int32_t* fcol,
                            const int32_t* fstart, const int32_t* fend, int64_t F, int64_t* removed_bp,
                            int32_t* genes_removed, uint64_t* signature, hipStream_t s) {
  if (n <= 0) return;
  const int64_t kb16 = (G + 127) / 128, wgs = (n + kMsRowsPerWg - 1) / kMsRowsPerWg;
  if (wgs > 0x7fffffff)
    throw Gm2Error("mask_minimized_stats: %lld rows are more workgroups than one launch holds", (long long)n);
  // (each wave's row in LDS when the four of a workgroup fit in 64 KB; else the gathers read global memory)
  const int64_t lds = 4 * kb16 * 16;
  if (lds <= 64 * 1024)
    hipLaunchKernelGGL(k_minimized_stats<true>, dim3((unsigned)wgs), dim3(256), (unsigned)lds, s, bits, n, ldb, (int)kb16,
                       (int)G, fcol, fstart, fend, (int)F, removed_bp, genes_removed, (unsigned long long*)signature);
  else
    hipLaunchKernelGGL(k_minimized_stats<false>, dim3((unsigned)wgs), dim3(256), 0, s, bits, n, ldb, (int)kb16, (int)G,
                       fcol, fstart, fend, (int)F, removed_bp, genes_removed, (unsigned long long*)signature);
  GM2_CHECK_LAUNCH();
}

void launch_count_groups(const uint8_t* bits, int64_t n, int64_t ldb, const int32_t* goff, int64_t ngroups,
                         const int32_t* pos, int32_t* counts, hipStream_t s) {
  if (n <= 0) return;
  // (whole-row form when the rows are 16-B pieces and the mask + list fit in 64 KB of LDS; each wave's
  // row buffer too when that still fits)
  const int64_t lds = ldb + (ngroups + 1) * 4;
  const int64_t lds_stage = ((lds + 15) & ~(int64_t)15) + 4 * ldb;
  if ((ldb & 15) == 0 && (((uintptr_t)bits) & 15) == 0 && lds <= 64 * 1024) {
    const int stage = lds_stage <= 64 * 1024 ? 1 : 0;
    hipLaunchKernelGGL(k_count_groups_rows, dim3((unsigned)((n + kCountRowsPerWg - 1) / kCountRowsPerWg)), dim3(256),
                       (unsigned)(stage ? lds_stage : lds), s, bits, n, ldb, goff, (int)ngroups, pos, counts, stage);
  } else {
    hipLaunchKernelGGL(k_count_groups, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, bits, n, ldb, goff,
                       (int)ngroups, pos, counts);
  }
  GM2_CHECK_LAUNCH();
}

void launch_row_offsets(const uint8_t* bits, int64_t n, int64_t ldb, const uint8_t* keep, int64_t* offsets,
                        hipStream_t s) {
  if (hipMemsetAsync(offsets, 0, sizeof(int64_t), s) != hipSuccess) throw Gm2Error("hipMemsetAsync");
  if (n <= 0) return;
  hipLaunchKernelGGL(k_row_popcount, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, bits, n, ldb, keep, offsets + 1);
  GM2_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_scan_inclusive, dim3(1), dim3(1024), 0, s, offsets + 1, n);
  GM2_CHECK_LAUNCH();
}

void launch_compact(const uint8_t* bits, int64_t n, int64_t ldb, const uint8_t* keep, const int64_t* offsets,
                    int32_t* idx, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_compact, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, bits, n, ldb, keep, offsets, idx);
  GM2_CHECK_LAUNCH();
}

#ifdef GM2_DEBUG
GM2_DBG_TAKE_FN(dbg_take_masks)
#endif

}  // namespace gm2
