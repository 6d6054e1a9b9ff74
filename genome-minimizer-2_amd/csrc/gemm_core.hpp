// MFMA GEMM for the VAE hot path: C[M,N] = sum_k P[m,k] * Q[n,k]  ("NT": both operands
// K-contiguous, the layout the 16x16 MFMA fragments read with one ds_read_b128 per lane).
//
//  * T = bf16_t : v_mfma_f32_16x16x32_bf16 (training fast path, fp32 accumulate)
//  * T = float  : v_mfma_f32_16x16x4_f32   (exact-f32 path: sampling decode + parity training)
//
// Tile configurations (Cfg<BM, BN, WGM, WGN>): a block of WGM x WGN waves owns a BM x BN output
// tile, each wave a (BM/WGM) x (BN/WGN) sub-tile of 16x16 MFMA fragments.
//   Big   256x256, 8 waves (2x4, 128x64 per wave): the G x H GEMMs (half the L2->LDS bytes per
//         FLOP of a 128x128 tile, which at full MFMA rate would need ~36 TB/s of L2 bandwidth).
//   Small 128x128, 4 waves (2x2, 64x64 per wave): the H x H / latent GEMMs.
// One K-step = one 128-byte row chunk per operand row (64 bf16 / 32 f32). Operands are staged
// HBM->LDS with global_load_lds_dwordx4 (no VGPR round trip) into a 2-stage ring; the LDS image
// is XOR-swizzled (chunk ^= (row>>1)&7) through the per-lane SOURCE address, which makes the
// 16-lane ds_read_b128 groups conflict-free.
// Block -> tile: 1-D grid, bijective XCD remap (consecutive logical tiles share an XCD's L2),
// then split-K slice outermost and GROUP_M=8 grouped (m fastest) tile order.
//
// Contract (checked on the host): every operand buffer has >= roundup(M|N, tile) rows, K is a
// multiple of 64, pads are zero.
//
// This header is the device code every kernel family shares (tile configurations, tile order,
// operand staging, fragments, both main loops); each family's epilogue, kernels and launchers are one
// translation unit: gemm_store.hip, gemm_recon.hip, gemm_mask.hip.
#pragma once
#include "gm2_common.hpp"
#include "gm2_kernels.hpp"

#include <algorithm>
#include <type_traits>

namespace gm2 {

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// Diagnostic timestamps (s_memrealtime, 100 MHz) of the store kernel's phases per workgroup; only
// compiled into the standalone probes under tools/probe, never into libgm2.
#ifdef GM2_STAMPS
__device__ unsigned long long g_stamp[16384][8];
#define GM2_STAMP(i) \
  if (threadIdx.x == 0) g_stamp[blockIdx.x][i] = __builtin_amdgcn_s_memrealtime()
#else
#define GM2_STAMP(i)
#endif

template <int BM_, int BN_, int WGM_, int WGN_, int NS_ = 2, int MINW_ = 1>
struct Cfg {
  static constexpr int MINW = MINW_;                 // min waves per SIMD (launch bounds: VGPR cap)
  static constexpr int BM = BM_, BN = BN_, WGM = WGM_, WGN = WGN_;
  static constexpr int NT = 64 * WGM * WGN;          // threads
  static constexpr int WTM = BM / WGM, WTN = BN / WGN;
  static constexpr int FM = WTM / 16, FN = WTN / 16;  // 16x16 fragments per wave
  static constexpr int STAGE = (BM + BN) * 128;      // bytes per pipeline stage
  static constexpr int NS = NS_;                     // pipeline stages in LDS
  static constexpr int LDS = NS * STAGE;
  static constexpr int LPS = (BM + BN) * 8 / NT;     // global_load_lds per thread per stage
};
using Big = Cfg<256, 256, 2, 4>;
using Small = Cfg<128, 128, 2, 2>;
// The fp32-output 128x128 tiles (hidden-layer GEMMs: one tile per CU, K = 1024 in 16 steps of
// ~0.2 us of MFMA each, against ~1 us from global_load_lds issue to landing): a 4-stage ring keeps
// three K-steps in flight instead of one.
using SmallDeep = Cfg<128, 128, 2, 2, 4>;
// The same tile with 8 waves (2x4, 64x32 each): two waves per SIMD, so one's LDS reads and waits
// hide behind the other's MFMAs (GM2_OPT_SMALL_WAVES = 8)
using SmallDeep8 = Cfg<128, 128, 2, 4, 4>;

struct TileXY {
  int m0, n0, split, t;
};

// XCD-aware, grouped tile order (see header)
__device__ __forceinline__ int xcd_wg(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
__device__ __forceinline__ int xcd_wg() { return xcd_wg(blockIdx.x, gridDim.x); }

// logical tile t (GROUP_M = 8 supergroups, m fastest) -> tile origin
template <class C>
__device__ __forceinline__ TileXY tile_at(int t, int tm, int tn, int split) {
  constexpr int GROUP = 8;
  const int per_group = GROUP * tn;
  const int grp = t / per_group;
  const int first_m = grp * GROUP;
  const int gsize = min(tm - first_m, GROUP);
  const int in = t - grp * per_group;
  const int pm = first_m + in % gsize;
  const int pn = in / gsize;
  return {pm * C::BM, pn * C::BN, split, pm * tn + pn};
}

template <class C>
__device__ __forceinline__ TileXY tile_of(int tm, int tn) {
  const int wg = xcd_wg();
  const int ntile = tm * tn;
  const int split = wg / ntile;
  return tile_at<C>(wg - split * ntile, tm, tn, split);
}

// ---- operand staging (HBM -> LDS with global_load_lds_dwordx4; LDS destination lane-linear) ----
// K-major operand (stored [rows][ld], K contiguous): the tile is ROWS rows x 128 B (one K-step);
// 16-B chunk c of row r lives at chunk position c ^ ((r>>1)&7)  -> conflict-free ds_read_b128.
template <class C, typename T, int ROWS>
__device__ __forceinline__ void stage_kmajor(const T* __restrict__ P, int64_t ldp, int row0, int k0, char* lds,
                                             int wid, int lane) {
  constexpr int EPC = 16 / sizeof(T);
  constexpr int PER = ROWS * 8 / C::NT;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = j * C::NT + wid * 64 + lane;
    const int row = i >> 3;
    const int c = (i & 7) ^ ((row >> 1) & 7);
    const T* src = P + (int64_t)(row0 + row) * ldp + k0 + c * EPC;
    __builtin_amdgcn_global_load_lds((const void*)src, (lds_void*)(lds + (j * C::NT + wid * 64) * 16), 16, 0, 0);
  }
}

// MN-major operand (stored [K][ld], its M or N dimension contiguous): the tile is KT k-rows x
// R elements; 16-B chunk c of k-row k lives at chunk position c ^ swz(k). swz keeps chunk pairs
// together and spreads the 8 k-rows one 32-lane half of a ds_read_b64_tr_b16 touches over 8
// distinct 32-B bank groups (conflict-free transposed reads).
__device__ __forceinline__ int swz_mn(int k) { return 2 * ((k & 3) | ((k >> 1) & 4)); }

template <class C, typename T, int R>
__device__ __forceinline__ void stage_mnmajor(const T* __restrict__ P, int64_t ldp, int col0, int k0, char* lds,
                                              int wid, int lane) {
  constexpr int EPC = 16 / sizeof(T);
  constexpr int CPR = R / EPC;                // chunks per k-row
  constexpr int PER = E<T>::KT * CPR / C::NT;
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = j * C::NT + wid * 64 + lane;
    const int k = i / CPR;
    const int c = (i % CPR) ^ swz_mn(k);
    const T* src = P + (int64_t)(k0 + k) * ldp + col0 + c * EPC;
    __builtin_amdgcn_global_load_lds((const void*)src, (lds_void*)(lds + (j * C::NT + wid * 64) * 16), 16, 0, 0);
  }
}

__device__ __forceinline__ int frag_off(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// bf16 fragment of operand rows [r0, r0+16) for k-substep s (32 k): lane l holds row r0 + (l&15),
// k = 32s + 8(l>>4) + j, j = 0..7 (the 16x16x32 MFMA A/B lane map).
template <bool KMAJ, int R>
__device__ __forceinline__ bf16x8 frag_bf16(const char* tile, int r0, int s, int lane) {
  if constexpr (KMAJ) {
    return *(const bf16x8*)(tile + frag_off(r0 + (lane & 15), s * 4 + (lane >> 4)));
  } else {
    constexpr int RB = R * 2;  // bytes per k-row
    const int i = lane & 15, q = i >> 2, p = i & 3;
    const int k = s * 32 + 8 * (lane >> 4) + q;
    const int c = (r0 >> 3) + (p >> 1);
    const char* a1 = tile + k * RB + ((c ^ swz_mn(k)) << 4) + (p & 1) * 8;
    const char* a2 = tile + (k + 4) * RB + ((c ^ swz_mn(k + 4)) << 4) + (p & 1) * 8;
    const bf16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a1);
    const bf16x4 v2 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)a2);
    return bf16x8{v1[0], v1[1], v1[2], v1[3], v2[0], v2[1], v2[2], v2[3]};
  }
}

// f32 fragment for k-substep s (16 k): lane l holds row r0 + (l&15), k = 16s + 4(l>>4) + j, j = 0..3
template <bool KMAJ, int R>
__device__ __forceinline__ f32x4 frag_f32(const char* tile, int r0, int s, int lane) {
  if constexpr (KMAJ) {
    return *(const f32x4*)(tile + frag_off(r0 + (lane & 15), s * 4 + (lane >> 4)));
  } else {
    constexpr int RB = R * 4;
    const int r = r0 + (lane & 15);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = s * 16 + 4 * (lane >> 4) + j;
      v[j] = *(const float*)(tile + k * RB + (((r >> 2) ^ swz_mn(k)) << 4) + (r & 3) * 4);
    }
    return v;
  }
}

// Wait until at most `r` (0 <= r <= NS - 2; negative = 0) later stages' loads are in flight.
template <class C>
__device__ __forceinline__ void wait_stages(int r) {
  static_assert(C::NS <= 5 && 3 * C::LPS <= 63, "vmcnt range");
  if (C::NS >= 5 && r >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * C::LPS) : "memory");
  else if (C::NS >= 4 && r >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * C::LPS) : "memory");
  else if (C::NS >= 3 && r >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(C::LPS) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Main loop. acc[mi][ni][j] = C[m0 + wm*WTM + mi*16 + 4*(lane>>4) + j][n0 + wn*WTN + ni*16 + (lane&15)]
// AK / BK: P / Q stored K-major (true) or MN-major (false).
template <class C, typename T, bool AK, bool BK>
__device__ __forceinline__ void mainloop(const T* __restrict__ P, int64_t ldp, const T* __restrict__ Q, int64_t ldq,
                                         int m0, int n0, int kbeg, int nk, char* smem,
                                         f32x4 (&acc)[C::FM][C::FN]) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / C::WGN, wn = wid % C::WGN;
  constexpr int KT = E<T>::KT;
#pragma unroll
  for (int a = 0; a < C::FM; ++a)
#pragma unroll
    for (int b = 0; b < C::FN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nk <= 0) return;

  auto stage = [&](char* buf, int k0) {
    if constexpr (AK) stage_kmajor<C, T, C::BM>(P, ldp, m0, k0, buf, wid, lane);
    else stage_mnmajor<C, T, C::BM>(P, ldp, m0, k0, buf, wid, lane);
    if constexpr (BK) stage_kmajor<C, T, C::BN>(Q, ldq, n0, k0, buf + C::BM * 128, wid, lane);
    else stage_mnmajor<C, T, C::BN>(Q, ldq, n0, k0, buf + C::BM * 128, wid, lane);
  };
  // NS-stage ring: K-step kt lives in buffer kt % NS; step kt + NS - 1 is issued at the top of
  // step kt into the buffer step kt - 1 used (every wave passed the barrier after reading it).
  // The wait at the end of step kt lets the stages after kt + 1 stay in flight (counted vmcnt).
  constexpr int NS = C::NS;
#pragma unroll
  for (int st = 0; st < NS - 1; ++st)
    if (st < nk) stage(smem + st * C::STAGE, kbeg + st * KT);
  wait_stages<C>(min(NS - 2, nk - 1));
  __syncthreads();
  GM2_STAMP(1);

  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt % NS) * C::STAGE;
    if (kt + NS - 1 < nk) stage(smem + ((kt + NS - 1) % NS) * C::STAGE, kbeg + (kt + NS - 1) * KT);
    const char* sA = cur;
    const char* sB = cur + C::BM * 128;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 b[C::FN];
#pragma unroll
        for (int ni = 0; ni < C::FN; ++ni) b[ni] = frag_bf16<BK, C::BN>(sB, wn * C::WTN + ni * 16, s, lane);
#pragma unroll
        for (int mi = 0; mi < C::FM; ++mi) {
          const bf16x8 a = frag_bf16<AK, C::BM>(sA, wm * C::WTM + mi * 16, s, lane);
#pragma unroll
          for (int ni = 0; ni < C::FN; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[ni], acc[mi][ni], 0, 0, 0);
        }
      }
    } else {
      // exact-fp32 path: each K-step's 32 products go into a fresh partial sum that is then added
      // to the accumulator, so a K-long dot product is a chain of K/32 additions of 32-term blocks
      // instead of one K-long fma chain. On the long-K GEMMs of the step (K = G = 55,040, the input
      // layer and the output layer's input gradient) this keeps the rounding error of the train-mode
      // BatchNorm backward's near-cancelling column sums at the level of the reference's own MKL
      // arithmetic (tools/diag/c3_chain.py: the single chain was 2.5-6x worse on the hidden layers)
      f32x4 part[C::FM][C::FN];
#pragma unroll
      for (int a = 0; a < C::FM; ++a)
#pragma unroll
        for (int b = 0; b < C::FN; ++b) part[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        f32x4 b[C::FN];
#pragma unroll
        for (int ni = 0; ni < C::FN; ++ni) b[ni] = frag_f32<BK, C::BN>(sB, wn * C::WTN + ni * 16, s, lane);
#pragma unroll
        for (int mi = 0; mi < C::FM; ++mi) {
          const f32x4 a = frag_f32<AK, C::BM>(sA, wm * C::WTM + mi * 16, s, lane);
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int ni = 0; ni < C::FN; ++ni)
              part[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[ni][j], part[mi][ni], 0, 0, 0);
        }
      }
#pragma unroll
      for (int mi = 0; mi < C::FM; ++mi)
#pragma unroll
        for (int ni = 0; ni < C::FN; ++ni) acc[mi][ni] += part[mi][ni];
    }
    wait_stages<C>(min(NS - 2, nk - 2 - kt));
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// Ping-pong main loop for the 256x256 bf16 tile (8 waves = two groups of four, one wave of each
// group per SIMD). Each K-tile (64 k) is consumed in 4 phases, one 64x32 quadrant of each wave's
// 128x64 sub-tile per phase (16 MFMAs): (a0,b0) (a0,b1) (a1,b0) (a1,b1), where a = which 64 of
// the wave's 128 rows and b = which 32 of its 64 columns. The stage of a K-tile is split into the
// four matching half-tiles, each its own 16 KB LDS region of the tile's buffer:
//   A_a : the rows {g*128 + a*64 + 0..63 : g = 0,1}   (both groups' a-halves)
//   B_b : the cols {w*64 + b*32 + 0..31 : w = 0..3}
// Phase p of tile t: [L] ds_read this quadrant's new fragments from buffer t&1, [G] issue one
// half-tile into buffer (t+1)&1 (A0, B0, B1, A1 of tile t+1 at p = 0..3; with kPPDeep, the
// default, B1(t+1), A1(t+1), A0(t+2), B0(t+2): each half-tile as early as the WAR rule allows),
// [W] counted vmcnt, barrier, MFMAs, barrier. Group 1 runs one barrier behind group 0, so on every SIMD one wave
// computes while the other reads LDS and issues loads (MI355X_MICROARCH.md "Two waves per SIMD").
// Ordering (barrier instances counted globally, phase n = 4t+p):
//  * RAW: a half-tile issued at phase n_i is covered by every wave's vmcnt at phase n_w and read
//    at phase >= n_w + 1: A0(t+1), B0(t+1) retired at 4t+3, read at 4(t+1); B1 issued 4t+2,
//    retired 4t+4, read 4t+5; A1 issued 4t+3, retired 4t+5, read 4t+6. Steady-state wait
//    vmcnt(4) = two later half-tiles x 2 loads per thread; none at p = 2.
//  * WAR: a region of buffer (t+1)&1 is restaged >= 4 phases after its last read in tile t-1
//    (the rule needs >= 2).
// ---------------------------------------------------------------------------------------------
// mainloop_pp issues each half-tile two phases earlier (DEEP below): 4-5 phases between issue and
// retire instead of 2-3, 8 loads in flight -- the 256-tile kernels are bound by that latency, not
// by their barriers or L2 -> LDS bytes (profiles/r04_pp_deep_prefetch_ab.txt: -50 us/step)
constexpr bool kPPDeep = true;
namespace pp {
constexpr int REGION = 128 * 128;  // bytes of one half-tile region (128 rows x 128 B, or 64 k x 256 B)
constexpr int BUF = 4 * REGION;    // one K-tile: A0, A1, B0, B1
// operand row pitch (elements) up to which a thread's 32-bit source offset holds (stage_half; check_gemm)
constexpr int64_t kPPMaxLd = int64_t(1) << 24;
__device__ __forceinline__ int a_row(int r, int a) { return (r >> 6) * 128 + a * 64 + (r & 63); }
__device__ __forceinline__ int b_row(int r, int b) { return (r >> 5) * 64 + b * 32 + (r & 31); }

// element offset from P of 16-B chunk i (0..1023) of half-tile `half` of the tile at (base, k0): the
// swizzled source of LDS position i (no row table)
template <bool KMAJ, bool ISA>
__device__ __forceinline__ int64_t chunk_off(int i, int64_t ld, int base, int half, int k0) {
  if constexpr (KMAJ) {
    const int row = i >> 3, c = (i & 7) ^ ((row >> 1) & 7);
    return (int64_t)(base + (ISA ? a_row(row, half) : b_row(row, half))) * ld + k0 + c * 8;
  } else {
    const int k = i >> 4, e = ((i & 15) ^ swz_mn(k)) * 8;
    return (int64_t)(k0 + k) * ld + base + (ISA ? a_row(e, half) : b_row(e, half));
  }
}

// one half-tile: 1024 16-B chunks, 2 per thread (lane-linear LDS destination, swizzled source);
// wave0 = the wave's first thread, wave-uniform.
// Without a row table chunk_off is a sum of a part that depends on the thread alone and a part that
// is the same for the whole block: chunk i = j*512 + tid has row (k-row) j*64 + (tid>>3) (j*32 +
// (tid>>4)); a_row / b_row send j*64 rows to j*128 and a half to +64 / +32 whatever the thread's
// bits are, and neither swizzle reads the bits j sets. So a load's address is a block-uniform base
// (tile, half, j, K-tile: scalar arithmetic) plus ONE loop-invariant 32-bit byte offset per thread and
// operand, and the one 64-bit add of the two is all the vector address arithmetic a load has left.
// Formed per chunk from chunk_off the main loop spent 34 (both K-major) to 65 (MN-major Q: a 64-bit
// (k0 + k) * ld per load) VALU instructions per wave and K-tile beside its 64 MFMAs, and held seven
// 64-bit pointers per thread; now 16 to 21 (profiles/r07_mn_major_b_ab.txt). The offset is below
// 128 rows * ld * 2 B + 256, so it fits for ld < kPPMaxLd (check_gemm).
// IDX (zero-copy rows): the thread's two rows (K-major) / k-rows (MN-major), j = 0, 1, are rr[j],
// read from the tile's LDS index table ahead of the issuing phase (idx_rows below)
template <bool KMAJ, bool ISA, bool IDX = false>
__device__ __forceinline__ void stage_half(const bf16_t* __restrict__ P, int64_t ld, int base, int half, int k0,
                                           char* region, int tid, int wave0, const int* rr = nullptr) {
  [[maybe_unused]] const uint32_t voff = 2u * (uint32_t)chunk_off<KMAJ, ISA>(tid, ld, 0, 0, 0);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = j * 512 + tid;
    const void* src;
    if constexpr (!IDX) {
      src = (const char*)(P + chunk_off<KMAJ, ISA>(j * 512, ld, base, half, k0)) + voff;
    } else {  // (table entries are >= 0 and ld < kPPMaxLd: one 32 x 32 -> 64-bit multiply per row)
      const uint64_t r = (uint64_t)(uint32_t)rr[j] * (uint32_t)ld;
      if constexpr (KMAJ) {
        const int row = i >> 3;
        const int c = (i & 7) ^ ((row >> 1) & 7);
        src = P + r + k0 + c * 8;
      } else {
        const int k = i >> 4;
        const int e = ((i & 15) ^ swz_mn(k)) * 8;
        src = P + r + base + (ISA ? a_row(e, half) : b_row(e, half));
      }
    }
    __builtin_amdgcn_global_load_lds(src, (lds_void*)(region + (j * 512 + wave0) * 16), 16, 0, 0);
  }
}

// the table entries of the thread's two rows of a K-major half-tile (tile-local rows a_row(.)) or
// of its two k-rows of an MN-major half-tile of K-tile t (table = the split's k-rows)
template <bool KMAJ>
__device__ __forceinline__ void idx_rows(const int* sidx, int half, int t, int tid, int (&rr)[2]) {
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = j * 512 + tid;
    if constexpr (KMAJ) rr[j] = sidx[a_row(i >> 3, half)];
    else rr[j] = sidx[t * 64 + (i >> 4)];
  }
}

__device__ __forceinline__ void barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}
}  // namespace pp

// S3 (the bf16x3 split decode): both operands in launch_split3's layout -- K-substep s = 0 of each
// K-tile is the hi part, s = 1 the lo part of the same 32 k -- and each fragment pair contributes
// hi.hi + hi.lo + lo.hi (three MFMAs instead of the two of a plain K-tile; lo.lo is dropped)
template <bool AK, bool BK, int IDX = 0, bool S3 = false>
__device__ __forceinline__ void mainloop_pp(const bf16_t* __restrict__ P, int64_t ldp, const bf16_t* __restrict__ Q,
                                            int64_t ldq, int m0, int n0, int kbeg, int nk, char* smem,
                                            f32x4 (&acc)[8][4], const int* sidx = nullptr) {
  // DEEP: the longer-prefetch issue order
  constexpr bool DEEP = kPPDeep;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  // wave-uniform in an SGPR: the stagger barriers below must be branched around, not exec-masked
  const int wm = __builtin_amdgcn_readfirstlane(wid >> 2), wn = wid & 3;
  const int wave0 = __builtin_amdgcn_readfirstlane(tid & ~63);
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (nk <= 0) return;
  // half-tile h (0 = A0, 1 = B0, 2 = B1, 3 = A1) of K-tile t -> its region
  auto region = [&](int t, int h) -> char* {
    const int off = h == 0 ? 0 : h == 3 ? 1 : h + 1;  // A0 0, A1 1, B0 2, B1 3
    return smem + (t & 1) * pp::BUF + off * pp::REGION;
  };
  // zero-copy rows: IDX 1 = P's rows (the tile's A rows: fixed, held for the tile), IDX 2 = Q's
  // k-rows (read one phase ahead of the two B-half issues of each K-tile, so the table read never
  // waits behind the phase's fragment reads)
  int ra0[2] = {0, 0}, ra1[2] = {0, 0}, rq[2] = {0, 0};
  if constexpr (IDX == 1) {
    pp::idx_rows<true>(sidx, 0, 0, tid, ra0);
    pp::idx_rows<true>(sidx, 1, 0, tid, ra1);
  }
  auto issue = [&](int t, int h) {
    const int k0 = kbeg + t * 64;
    char* r = region(t, h);
    if (h == 0 || h == 3) pp::stage_half<AK, true, IDX == 1>(P, ldp, m0, h == 0 ? 0 : 1, k0, r, tid, wave0, h == 0 ? ra0 : ra1);
    else pp::stage_half<BK, false, IDX == 2>(Q, ldq, n0, h == 1 ? 0 : 1, k0, r, tid, wave0, rq);
  };
  bf16x8 fa[4][2], fb0[2][2], fb1[2][2];
  auto read_a = [&](int t, int a) {
    const char* r = region(t, a == 0 ? 0 : 3);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int s = 0; s < 2; ++s) fa[mi][s] = frag_bf16<AK, 128>(r, wm * 64 + mi * 16, s, lane);
  };
  auto read_b = [&](int t, int b, bf16x8 (&fb)[2][2]) {
    const char* r = region(t, b == 0 ? 1 : 2);
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int s = 0; s < 2; ++s) fb[ni][s] = frag_bf16<BK, 128>(r, wn * 32 + ni * 16, s, lane);
  };
  auto mma = [&](int a, int b, const bf16x8 (&fb)[2][2]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        f32x4& c = acc[a * 4 + mi][b * 2 + ni];
        if constexpr (S3) {
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mi][0], fb[ni][0], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mi][0], fb[ni][1], c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mi][1], fb[ni][0], c, 0, 0, 0);
        } else {
#pragma unroll
          for (int s = 0; s < 2; ++s) c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[mi][s], fb[ni][s], c, 0, 0, 0);
        }
      }
    __builtin_amdgcn_s_setprio(0);
  };
  // prologue: all four half-tiles of tile 0; A0, B0 retired before the first reads
  if constexpr (IDX == 2) pp::idx_rows<false>(sidx, 0, 0, tid, rq);
  if constexpr (DEEP) {  // tile 0, then A0 and B0 of tile 1 (issued at phases 2 and 3 of tile -1)
#pragma unroll
    for (int h = 0; h < 4; ++h) issue(0, h);
    if (nk > 1) {
      issue(1, 0);
      if constexpr (IDX == 2) pp::idx_rows<false>(sidx, 0, 1, tid, rq);
      issue(1, 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // A0(0), B0(0)
    } else {
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    }
  } else {
#pragma unroll
    for (int h = 0; h < 4; ++h) issue(0, h);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  }
  pp::barrier();
  GM2_STAMP(1);
  if (wm == 1) pp::barrier();  // stagger: group 1 one barrier behind
  if constexpr (DEEP) {
    // Issue order two phases earlier than below (each half-tile as soon as the WAR rule allows):
    // tile t issues B1(t+1) at phase 0, A1(t+1) at 1, A0(t+2) at 2, B0(t+2) at 3, so every half-tile
    // has four to five phases between its issue and its retire (two to three below). Retire points
    // are unchanged: B1(t) at phase 0, A1(t) at 1, A0 / B0 (t+1) at 3; 8 loads stay in flight.
    int rq2[2] = {0, 0};  // IDX 2: the k-rows of B0(t+2), read at phase 1
    for (int t = 0; t < nk; ++t) {
      const bool m1 = t + 1 < nk, m2 = t + 2 < nk;
      if constexpr (IDX == 2) {
        if (m1) pp::idx_rows<false>(sidx, 0, t + 1, tid, rq);  // B1(t+1)
      }
      // phase 0: (a0, b0)
      read_a(t, 0);
      read_b(t, 0, fb0);
      if (m1) {
        issue(t + 1, 2);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // retires B1(t)
      } else {
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      }
      pp::barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      mma(0, 0, fb0);
      pp::barrier();
      // phase 1: (a0, b1)
      read_b(t, 1, fb1);
      if constexpr (IDX == 2) {
        if (m2) pp::idx_rows<false>(sidx, 0, t + 2, tid, rq2);
      }
      if (m1) {
        issue(t + 1, 3);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // retires A1(t)
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      pp::barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      mma(0, 1, fb1);
      pp::barrier();
      // phase 2: (a1, b0)
      read_a(t, 1);
      if (m2) issue(t + 2, 0);
      pp::barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      mma(1, 0, fb0);
      pp::barrier();
      // phase 3: (a1, b1)
      if (m2) {
        if constexpr (IDX == 2) {
          rq[0] = rq2[0];
          rq[1] = rq2[1];
        }
        issue(t + 2, 1);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // retires A0(t+1), B0(t+1)
      } else if (m1) {
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      }
      pp::barrier();
      __builtin_amdgcn_sched_barrier(0);
      mma(1, 1, fb1);
      pp::barrier();
    }
  } else {
    for (int t = 0; t < nk; ++t) {
      const bool more = t + 1 < nk;
      if constexpr (IDX == 2) {
        if (more) pp::idx_rows<false>(sidx, 0, t + 1, tid, rq);
      }
      // phase 0: (a0, b0)
      read_a(t, 0);
      read_b(t, 0, fb0);
      if (more) {
        issue(t + 1, 0);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // retires B1(t)
      } else {
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      }
      pp::barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      mma(0, 0, fb0);
      pp::barrier();
      // phase 1: (a0, b1)
      read_b(t, 1, fb1);
      if (more) {
        issue(t + 1, 1);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // retires A1(t)
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      pp::barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      mma(0, 1, fb1);
      pp::barrier();
      // phase 2: (a1, b0)
      read_a(t, 1);
      if (more) issue(t + 1, 2);
      pp::barrier();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      mma(1, 0, fb0);
      pp::barrier();
      // phase 3: (a1, b1)
      if (more) {
        issue(t + 1, 3);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // retires A0(t+1), B0(t+1)
      }
      pp::barrier();
      __builtin_amdgcn_sched_barrier(0);
      mma(1, 1, fb1);
      pp::barrier();
    }
  }
  if (wm == 0) pp::barrier();  // re-align the groups
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

}  // namespace

}  // namespace gm2
