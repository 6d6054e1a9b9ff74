// The sampling-decode mask GEMM family (gemm_core.hpp): epilogue 3 with the certified band,
// k_gemm_mask, k_gemm_mask_tiered and their launchers.
#include "gemm_launch.hpp"

namespace gm2 {

namespace {

// ---------------------------------------------------------------------------------------------
// Epilogue 3: sampling / evaluation output layer. pred = sigmoid_fp32(logit) > thr: for thr = 0.5
// (the reference's extras.py:200-201 `> 0.5`) as logit > 0x33C00000, else p > thr with
// p = 1 / (1 + exp(-logit)) in fp32. The tile's predictions go through an LDS u8 image and leave as
//   * mask  u8 [m][ldm] (full-row byte runs; 16-byte stores when ldm allows), and/or
//   * bits  [m][ldb] bytes, numpy packbits(bitorder='little') rows: bit (n & 7) of byte n / 8, and/or
//   * counts int32 [m][3] += (TP, FP, FN) against the row-major target bits (metrics.py:19-64), and/or
//   * probs fp32 [m][ldpr] = p (extras.py:198).
// ---------------------------------------------------------------------------------------------

// The certified band (MaskBand): the tile's row norms and column norms go to LDS past the staging
// ring after the main loop (mask_tile), with the tile's slot counter after them. Per element the
// epilogues add one compare (|d| <= rmax * ce + eb, MaskBand) and its wave ballot: the packed-bits
// epilogue appends a position's flagged (row, gene) pairs right there (a uniform branch, rarely
// taken); the u8 epilogue ORs the ballots and a flagged wave re-walks its fragments.
template <class C>
constexpr int band_lds_bytes() { return (C::BM + C::BN) * 4 + 16; }

// the band's per-column terms of one lane (column fragment ni): bt = b - T, ce = coef ||w_g||
// (rounded up); the rounding floor 2^-21 (|b| + T) <= 2^-21 |bt| + 2^-20 T is formed per fragment.
// Pad genes: bt = -inf, ce = -inf (never in the band)
template <class C>
struct BandCols {
  float bt[C::FN], ce[C::FN];
  __device__ __forceinline__ BandCols(const float* __restrict__ bias, const float* brn, const MaskBand& band, bool bchk,
                                      int n0, int N, int lane, int wn) {
#pragma unroll
    for (int ni = 0; ni < C::FN; ++ni) {
      const int nl = wn * C::WTN + ni * 16 + (lane & 15);
      const bool in = n0 + nl < N;
      bt[ni] = in ? bias[n0 + nl] - kMaskLogitThreshold : -INFINITY;
      ce[ni] = !in ? -INFINITY : bchk ? band.coef * brn[C::BM + nl] * (1.0f + 0x1p-20f) : 0.f;
    }
  }
  // this lane's band half-widths for row fragment mi (the largest of its four rows' norms); without
  // a band check: -1 (nothing is in it)
  __device__ __forceinline__ void widths(const float* brn, bool bchk, int r0, float (&e)[C::FN]) const {
    if (!bchk) {
#pragma unroll
      for (int ni = 0; ni < C::FN; ++ni) e[ni] = -1.f;
      return;
    }
    const float4 r4 = *(const float4*)(brn + r0);
    const float rmax = fmaxf(fmaxf(r4.x, r4.y), fmaxf(r4.z, r4.w));
#pragma unroll
    for (int ni = 0; ni < C::FN; ++ni)
      e[ni] = fmaf(rmax, ce[ni], fmaf(0x1p-21f, fabsf(bt[ni]), 0x1p-20f * kMaskLogitThreshold));
  }
};

// A band entry past its shard's capacity only sets the lane's `ovf`; after its epilogue the tile
// flags the 256 x 256 block it lies in (the first lane to flag it lists it) for k_band_tile_fix's
// whole-block fp64 recompute. (Flagging at each of the unrolled epilogue's 128 append sites had grown
// the bit-packing mask kernel from 120 to 208 KB of code and its launch from 5.0 to 5.7 ms; deferring
// every append to one rolled loop, 49 KB, measured 5.4 ms: profiles/r06_mask_code_size_ab.txt.)
__device__ __forceinline__ void band_spill_block(const MaskBand& b, int m0, int n0) {
  const unsigned blk = (unsigned)(m0 >> 8) * (unsigned)b.obn + (unsigned)(n0 >> 8);
  GM2_DBG(blk < b.oblocks && (n0 >> 8) < b.obn, kDbgBandBlock);
  if (blk >= b.oblocks) return;  // (cannot happen: tiles lie inside the block grid)
  if (atomicExch(b.oflag + blk, 1u) == 0u) b.olist[atomicAdd(b.ocount, 1u)] = blk;
}

// where a workgroup's band elements go: the tile's slot counter in LDS, its shard and the shard's list
struct BandDst {
  unsigned* lcount;
  int sh;
  uint2* shard;
};
template <class C>
__device__ __forceinline__ BandDst band_dst(const MaskBand& b, char* smem) {
  const int sh = blockIdx.x % kBandShards;
  return {(unsigned*)(smem + C::LDS) + C::BM + C::BN, sh, b.list + (size_t)sh * b.cap};
}
// one fragment position's band elements (bal = the wave's non-zero ballot of `in`; wave-uniform
// call): one reservation for all of them (an LDS counter for the tile's slots, else the shard's
// counter) and each flagged lane's entry at its prefix
__device__ __forceinline__ void band_add(const MaskBand& b, int tile, const BandDst& d, int lane, uint64_t bal, bool in,
                                         int r, int gcol, bool& ovf) {
  const unsigned pre = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
  unsigned base = 0;
  if (lane == 0) base = atomicAdd(b.tslots ? d.lcount : b.counts + d.sh, (unsigned)__popcll(bal));
  const unsigned i = __shfl(base, 0, 64) + pre;
  if (!in) return;
  const uint2 e = make_uint2((unsigned)r, (unsigned)gcol);
  if (!b.tslots) {
    if (i < b.cap) d.shard[i] = e;
    else ovf = true;
  } else if (i < (unsigned)b.tslots) {
    b.tlist[(size_t)tile * b.tslots + i] = e;
  } else if (!b.drop_overflow) {  // past the tile's slots: the shard (rare)
    const unsigned k = atomicAdd(b.counts + d.sh, 1u);
    if (k < b.cap) d.shard[k] = e;
    else ovf = true;
  }
}
// one wave's band elements: walk(visit) calls visit(in, row, gene) for every fragment position in a
// fixed order, and each position with flagged lanes appends them (band_add)
template <class C, class F>
__device__ __forceinline__ void band_walk(const MaskBand& b, int tile, char* smem, int lane, bool& ovf, F&& walk) {
  const BandDst d = band_dst<C>(b, smem);
  walk([&](bool in, int r, int gcol) {
    const uint64_t bal = __ballot(in);
    if (bal) band_add(b, tile, d, lane, bal, in, r, gcol, ovf);
  });
}

// after the epilogue's barrier: the tile's slot count
template <class C>
__device__ __forceinline__ void band_close(const MaskBand& b, int tile, char* smem) {
  if (!b.tslots || threadIdx.x != 0) return;
  const unsigned n = ((const unsigned*)(smem + C::LDS))[C::BM + C::BN];
  b.tcount[tile] = n;
  if (b.drop_overflow && n > (unsigned)b.tslots) return;  // (re-run by the split kernel, counted there)
  if (n) atomicAdd(b.tfound + blockIdx.x % kBandShards, min(n, (unsigned)b.tslots));
  if (b.tiles_done) atomicAdd(b.tiles_done + blockIdx.x % kSplitShards, 1u);
}

template <class C, typename T, bool PP, bool BITS, bool S3>
__device__ __forceinline__ void mask_tile(const TileXY tl, const GemmArgs<T>& g, const float* __restrict__ bias,
                                          const MaskOut& o, char* smem);

// PP: the 256x256 bf16 ping-pong main loop in its S3 form (the bf16x3 sampling decode: hi.hi +
// hi.lo + lo.hi over operands split by launch_split3, K' = 2H, decode_split3). LOOP (gated 128 x
// 128 launches, usually the complement of the split kernel with few tiles to run): a grid of a few
// workgroups per CU loops over the tiles t, t + grid, ... instead of one workgroup per tile.
template <class C, typename T, bool PP = false, bool BITS = false, bool LOOP = false, bool S3 = true>
__global__ __launch_bounds__(C::NT) void k_gemm_mask(GemmArgs<T> g, const float* __restrict__ bias, MaskOut o) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tm = g.Mp / C::BM, tn = g.Np / C::BN, ntile = tm * tn;
  if constexpr (!LOOP) {
    const TileXY tl = tile_of<C>(tm, tn);
    if (o.gate.run) {  // the verdict of the tile's 256 x 256 block (uniform per workgroup)
      if (tile_level(o.gate, tl.m0, tl.n0) != o.gate.run) return;  // (tcount: zeroed by the caller)
      if (threadIdx.x == 0) atomicAdd(o.gate.tiles + blockIdx.x % kSplitShards, 1u);
    }
    mask_tile<C, T, PP, BITS, S3>(tl, g, bias, o, smem);
  } else {
    static_assert(!PP && !BITS, "tile loop: the 128 x 128 kernel");
    // the workgroup's tiles t0 + k G: their gate verdicts NT at a time, in parallel (one ballot word
    // per wave in LDS past the band region), then the runnable ones in order
    const int G = gridDim.x, t0 = xcd_wg(), lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t* vm = (uint64_t*)(smem + C::LDS + band_lds_bytes<C>());
    for (int kb = 0; t0 + kb * G < ntile; kb += C::NT) {
      __syncthreads();  // (the previous pass's words are read)
      const int t = t0 + (kb + (int)threadIdx.x) * G;
      bool run = false;
      if (t < ntile) {
        const TileXY tl = tile_at<C>(t, tm, tn, 0);
        run = !o.gate.run || tile_level(o.gate, tl.m0, tl.n0) == o.gate.run;
      }
      const uint64_t bw = __ballot(run);
      if (lane == 0) vm[wid] = bw;
      __syncthreads();
      unsigned nrun = 0;
#pragma unroll 1
      for (int w = 0; w < C::NT / 64; ++w) {
        const uint64_t v = vm[w];
        uint64_t m = ((uint64_t)__builtin_amdgcn_readfirstlane((unsigned)(v >> 32)) << 32) |
                     __builtin_amdgcn_readfirstlane((unsigned)v);
        while (m) {
          const int i = __builtin_ctzll(m);
          m &= m - 1;
          ++nrun;
          __syncthreads();  // (the previous tile's epilogue is done with LDS)
          mask_tile<C, T, PP, BITS, S3>(tile_at<C>(t0 + (kb + w * 64 + i) * G, tm, tn, 0), g, bias, o, smem);
        }
      }
      if (o.gate.run && nrun && threadIdx.x == 0) atomicAdd(o.gate.tiles + blockIdx.x % kSplitShards, nrun);
    }
  }
}

// The tiered output layer (GM2_OPT_SAMPLE_SINGLE): one 256x256 workgroup per tile takes its block's
// verdict -- exact tiles return at once (the exact kernel's), single-product tiles run one bf16
// product over the rounded operands (o1: K = H, the wide band, overflow dropped) and, when their band
// overflowed its slots, the same tile again as bf16x3 (o3) in place; split tiles run bf16x3 alone.
// One launch for both bf16 tiers: no second grid of workgroups that mostly exit.
template <class C, typename T, bool BITS>
__global__ __launch_bounds__(C::NT) void k_gemm_mask_tiered(GemmArgs<T> g1, GemmArgs<T> g3,
                                                            const float* __restrict__ bias, MaskOut o1, MaskOut o3) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const TileXY tl = tile_of<C>(g3.Mp / C::BM, g3.Np / C::BN);
  const int lv = tile_level(o3.gate, tl.m0, tl.n0);
  if (lv == 2) return;
  if (lv == 3) {
    mask_tile<C, T, true, BITS, false>(tl, g1, bias, o1, smem);
    __syncthreads();  // (band_close's count in LDS, read by every thread)
    if (((const unsigned*)(smem + C::LDS))[C::BM + C::BN] <= (unsigned)o1.band.tslots) return;  // (counted)
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(o3.gate.tiles + blockIdx.x % kSplitShards, 1u);
  mask_tile<C, T, true, BITS, true>(tl, g3, bias, o3, smem);
}

template <class C, typename T, bool PP, bool BITS, bool S3>
__device__ __forceinline__ void mask_tile(const TileXY tl, const GemmArgs<T>& g, const float* __restrict__ bias,
                                          const MaskOut& o, char* smem) {
  const bool bchk = o.band.rn != nullptr;
  // the tile's row and column norms (one per thread: NT = BM + BN), loaded before the main loop and
  // staged to LDS after it (its first counted wait covers the load; no stall in front of the loop)
  static_assert(C::NT == C::BM + C::BN, "one norm per thread");
  float nrm = 0.f;
  if (bchk) nrm = threadIdx.x < C::BM ? o.band.rn[tl.m0 + threadIdx.x] : o.band.cn[tl.n0 + threadIdx.x - C::BM];
  const float* brn = (const float*)(smem + C::LDS);  // [BM] row norms, then [BN] column norms
  f32x4 acc[C::FM][C::FN];
  if constexpr (PP) {
    static_assert(std::is_same_v<C, Big> && sizeof(T) == 2, "ping-pong: 256x256 bf16");
    // (S3: the split's K' = 2H form; else one product over K = H, the single-product tier)
    mainloop_pp<true, true, 0, S3>(g.P, g.ldp, g.Q, g.ldq, tl.m0, tl.n0, 0, g.K / E<T>::KT, smem, acc);
  } else {
    mainloop<C, T, true, true>(g.P, g.ldp, g.Q, g.ldq, tl.m0, tl.n0, 0, g.K / E<T>::KT, smem, acc);
  }
  if (bchk) {
    ((float*)(smem + C::LDS))[threadIdx.x] = nrm;
    if (threadIdx.x == 0) ((unsigned*)(smem + C::LDS))[C::BM + C::BN] = 0u;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wm = wid / C::WGN, wn = wid % C::WGN;
  const BandCols<C> bc(bias, brn, o.band, bchk, tl.n0, g.N, lane, wn);
  uint64_t bandw = 0;  // this wave's band flags, OR-ed over its fragment positions
  bool ovf = false;    // an entry of this lane's found its shard full (band_spill_block)
  if constexpr (BITS) {
    static_assert(PP, "bit-image epilogue: the split decode's kernel");
    {
      // packed bits straight from the fragments: lane l of a 16x16 fragment holds row 4(l>>4) + j,
      // column l&15, so one ballot per (mi, ni, j) yields 16 gene bits for each of 4 rows; lane r < 4
      // gathers row r's 64 bits over the wave's 4 column fragments and writes them to a [BM][32 B]
      // bit image (one ds_write_b64 per (mi, j), where the u8 image took one byte store per logit).
      // The bit is d = acc + (b - T) > 0 (pad genes: d = -inf); d and acc + b round differently
      // only inside the band, which the recompute decides.
      const int sh = 16 * (lane & 3);
#pragma unroll
      for (int mi = 0; mi < C::FM; ++mi) {
        float e[C::FN];
        bc.widths(brn, bchk, wm * C::WTM + mi * 16 + 4 * (lane >> 4), e);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          uint64_t rb = 0;
          const int r = tl.m0 + wm * C::WTM + mi * 16 + 4 * (lane >> 4) + j;
          const bool rok = r < g.M;
#pragma unroll
          for (int ni = 0; ni < C::FN; ++ni) {
            const float d = acc[mi][ni][j] + bc.bt[ni];
            const uint64_t bal = __ballot(d > 0.f);
            rb |= ((bal >> sh) & 0xFFFFull) << (16 * ni);
            // the band elements of this position appended at once (a uniform branch, rarely taken)
            const bool inb = fabsf(d) <= e[ni] && rok;
            const uint64_t bb = __ballot(inb);
            if (bb)
              band_add(o.band, tl.t, band_dst<C>(o.band, smem), lane, bb, inb, r,
                       tl.n0 + wn * C::WTN + ni * 16 + (lane & 15), ovf);
          }
          if (lane < 4)
            *(uint64_t*)(smem + (wm * C::WTM + mi * 16 + 4 * lane + j) * (C::BN / 8) + wn * (C::WTN / 8)) = rb;
          __builtin_amdgcn_sched_barrier(0);  // (one row quad at a time: the ballots' SGPR pairs stay few)
        }
      }
      if (ovf) band_spill_block(o.band, tl.m0, tl.n0);
      __syncthreads();
      band_close<C>(o.band, tl.t, smem);
      constexpr int BPR = C::BN / 8;
      const int rows = min(C::BM, g.M - tl.m0);
      if (o.bits) {
        for (int i = threadIdx.x; i < rows * (BPR / 16); i += C::NT) {
          const int r = i / (BPR / 16), cc = i % (BPR / 16);
          if (tl.n0 / 8 + cc * 16 >= o.ldb) continue;  // (pad genes past the row pitch: all zero)
          *(uint4*)(o.bits + (int64_t)(tl.m0 + r) * o.ldb + tl.n0 / 8 + cc * 16) = *(const uint4*)(smem + r * BPR + cc * 16);
        }
      }
      return;
    }
  }
  constexpr int PI = C::BN + 16;  // u8 image pitch
  uint8_t* img = (uint8_t*)smem;  // [BM][PI] (mainloop staging is free after its last barrier)
  const bool half = o.thr == 0.5f;
#pragma unroll
  for (int mi = 0; mi < C::FM; ++mi) {
    float e[C::FN];
    bc.widths(brn, bchk, wm * C::WTM + mi * 16 + 4 * (lane >> 4), e);
#pragma unroll
    for (int ni = 0; ni < C::FN; ++ni) {
      const int nl = wn * C::WTN + ni * 16 + (lane & 15);
      const int n = tl.n0 + nl;
      const float bnv = n < g.N ? bias[n] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ml = wm * C::WTM + mi * 16 + 4 * (lane >> 4) + j;
        const int m = tl.m0 + ml;
        const float l = acc[mi][ni][j] + bnv;
        float p = 0.f;
        if (o.probs || !half) p = 1.0f / (1.0f + expf(-l));
        const bool pred = n < g.N && (half ? l > kMaskLogitThreshold : p > o.thr);
        img[ml * PI + nl] = pred ? 1 : 0;
        if (o.probs && m < g.M && n < g.N) o.probs[(int64_t)m * o.ldpr + n] = p;
        if (bchk) bandw |= __ballot(fabsf(acc[mi][ni][j] + bc.bt[ni]) <= e[ni]);
      }
    }
  }
  if (bandw) {  // append this wave's band elements (unrolled: acc stays in registers)
    band_walk<C>(o.band, tl.t, smem, lane, ovf, [&](auto&& visit) {
#pragma unroll
      for (int mi = 0; mi < C::FM; ++mi) {
        float e[C::FN];
        bc.widths(brn, bchk, wm * C::WTM + mi * 16 + 4 * (lane >> 4), e);
#pragma unroll
        for (int ni = 0; ni < C::FN; ++ni)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int ml = wm * C::WTM + mi * 16 + 4 * (lane >> 4) + j;
            visit(fabsf(acc[mi][ni][j] + bc.bt[ni]) <= e[ni] && tl.m0 + ml < g.M, tl.m0 + ml,
                  tl.n0 + wn * C::WTN + ni * 16 + (lane & 15));
          }
      }
    });
  }
  if (ovf) band_spill_block(o.band, tl.m0, tl.n0);
  __syncthreads();
  band_close<C>(o.band, tl.t, smem);
  const int rows = min(C::BM, g.M - tl.m0);
  if (o.mask) {
    // one row per 8 threads' 16-byte pieces (or byte runs when the rows are not 16-B aligned)
    const bool vec = (o.ldm & 15) == 0 && (((uintptr_t)o.mask) & 15) == 0 && tl.n0 + C::BN <= g.N;
    if (vec) {
      constexpr int CPR = C::BN / 16;
      for (int i = threadIdx.x; i < rows * CPR; i += C::NT) {
        const int r = i / CPR, cc = i % CPR;
        *(uint4*)(o.mask + (int64_t)(tl.m0 + r) * o.ldm + tl.n0 + cc * 16) = *(const uint4*)(img + r * PI + cc * 16);
      }
    } else {
      const int cols = min(C::BN, g.N - tl.n0);
      for (int i = threadIdx.x; i < rows * C::BN; i += C::NT) {
        const int r = i / C::BN, cc = i % C::BN;
        if (cc < cols) o.mask[(int64_t)(tl.m0 + r) * o.ldm + tl.n0 + cc] = img[r * PI + cc];
      }
    }
  }
  if (o.bits) {
    // 8 image bytes -> one packed byte; BN / 8 bytes per row, written 16 at a time
    constexpr int BPR = C::BN / 8;
    static_assert(BPR % 16 == 0, "packed row piece");
    for (int i = threadIdx.x; i < rows * (BPR / 16); i += C::NT) {
      const int r = i / (BPR / 16), cc = i % (BPR / 16);
      if (tl.n0 / 8 + cc * 16 >= o.ldb) continue;  // (pad genes past the row pitch: all zero)
      uint32_t w[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint2 e = *(const uint2*)(img + r * PI + cc * 128 + (k * 4 + b) * 8);
          const uint32_t lo = e.x * 0x10204080u, hi = e.y * 0x10204080u;  // gather byte LSBs
          v |= (((lo >> 28) | ((hi >> 28) << 4)) & 0xFFu) << (8 * b);
        }
        w[k] = v;
      }
      *(uint4*)(o.bits + (int64_t)(tl.m0 + r) * o.ldb + tl.n0 / 8 + cc * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
  if (o.counts) {
    // per-row TP / FP / FN of this tile against the target bits; integer atomics (exact)
    constexpr int WPR = C::BN / 32;  // target words per tile row
    for (int i = threadIdx.x; i < rows * WPR; i += C::NT) {
      const int r = i / WPR, k = i % WPR;
      uint32_t pw = 0;
#pragma unroll
      for (int b = 0; b < 32; ++b) pw |= (uint32_t)img[r * PI + k * 32 + b] << b;
      const uint32_t xw = o.xbits[(int64_t)(tl.m0 + r) * o.ldxb + (tl.n0 >> 5) + k];
      int* cr = o.counts + (int64_t)(tl.m0 + r) * 3;
      const int tp = __builtin_popcount(pw & xw), fp = __builtin_popcount(pw & ~xw), fn = __builtin_popcount(~pw & xw);
      if (tp) atomicAdd(cr + 0, tp);
      if (fp) atomicAdd(cr + 1, fp);
      if (fn) atomicAdd(cr + 2, fn);
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
// a 256x256 launch writes packed bits at threshold 0.5 and nothing else (the ballot epilogue)
static bool bits_only(const MaskOut& o) { return o.bits && !o.mask && !o.probs && !o.counts && o.thr == 0.5f; }

void launch_gemm_mask_tiered(const GemmArgs<bf16_t>& g1, const GemmArgs<bf16_t>& g3, const float* bias,
                             const MaskOut& o1, const MaskOut& o3, hipStream_t s) {
  check_gemm(g1, 256);
  check_gemm(g3, 256);
  if (g1.Mp != g3.Mp || g1.Np != g3.Np || g1.Mp % 256 || g1.Np % 256 || g1.K % 64 || g3.K % 64)
    throw Gm2Error("tiered mask: the two GEMMs' tile grids differ");
  if (!bits_only(o1) || !bits_only(o3) || o1.bits != o3.bits || o1.ldb != o3.ldb)
    throw Gm2Error("tiered mask: both tiers write the same packed bits (threshold 0.5) and nothing else");
  check_bits_pitch(o3.bits, o3.ldb, g3.N);
  const MaskBand &band1 = o1.band, &band3 = o3.band;
  if (!band1.rn || !band3.rn || !band1.tslots || !band3.tslots || !band1.drop_overflow || !o3.gate.run)
    throw Gm2Error("tiered mask: both bands with tile slots (the single tier's dropping its overflow) and the gate");
  if (!band3.oflag || !band3.olist || !band3.ocount || band3.obn < g3.Np / 256 ||
      band3.oblocks < (unsigned)((g3.Mp / 256) * band3.obn))
    throw Gm2Error("tiered mask: the overflow block flags, list and counter required");
  constexpr int lds = Big::LDS + band_lds_bytes<Big>();
  TimedLaunch tl(kKcMask, s);
  launch_lds(k_gemm_mask_tiered<Big, bf16_t, true>, (g3.Mp / 256) * (g3.Np / 256), Big::NT, lds, lds, s, g1, g3, bias,
             o1, o3);
  GM2_CHECK_LAUNCH();
}

template <typename T>
void launch_gemm_mask(const GemmArgs<T>& g, const float* bias, const MaskOut& o, bool big, hipStream_t s) {
  const MaskBand& band = o.band;
  check_gemm(g, big ? 256 : 128);
  // (the 256-column tiles may reach past the row pitch: their bits stores stop at ldb, past G)
  check_bits_pitch(o.bits, o.ldb, big ? g.N : g.Np);
  if (o.counts && (!o.xbits || o.ldxb * 32 < g.Np)) throw Gm2Error("mask counts: target bits required");
  if (band.rn && (!band.cn || !band.counts || !band.list || !band.cap || o.thr != 0.5f))
    throw Gm2Error("mask band: norms, counter and list required (threshold 0.5 only)");
  if (band.rn && (!band.oflag || !band.olist || !band.ocount || band.obn < (g.Np + 255) / 256 ||
                  band.oblocks < (unsigned)(((g.Mp + 255) / 256) * band.obn)))
    throw Gm2Error("mask band: the overflow block flags, list and counter required");
  if (band.tslots && (!band.tlist || !band.tcount || !band.tfound || !big))
    throw Gm2Error("mask band: tile slots need their list, counters and the 256 x 256 kernel");
  const int band_lds = band.rn ? (big ? band_lds_bytes<Big>() : band_lds_bytes<Small>()) : 0;  // (norms + slot counter)
  TimedLaunch tl(kKcMask, s);
  if constexpr (sizeof(T) == 2) {
    if (big) {
      if (g.Mp % 256 || g.Np % 256 || g.K % 64) throw Gm2Error("mask (256x256): padded extents");
      if (!bits_only(o)) throw Gm2Error("mask (256x256): packed bits at threshold 0.5 only");
      constexpr int lds_max = Big::LDS + band_lds_bytes<Big>();
      launch_lds(k_gemm_mask<Big, T, true, true>, (g.Mp / 256) * (g.Np / 256), Big::NT, lds_max, Big::LDS + band_lds, s,
                 g, bias, o);
      GM2_CHECK_LAUNCH();
      return;
    }
  }
  if (big) throw Gm2Error("mask (256x256): bf16 only");
  static_assert(Small::LDS >= 128 * (128 + 16), "u8 image inside the staging ring");
  const int ntile = (g.Mp / 128) * (g.Np / 128);
  if (o.gate.run) {  // (the tile loop, from a grid of at most 1024 workgroups)
    // (LDS: the band region always, then the verdict words)
    constexpr int lds = Small::LDS + band_lds_bytes<Small>() + (Small::NT / 64) * 8;
    launch_lds(k_gemm_mask<Small, T, false, false, true>, std::min(ntile, 1024), Small::NT, lds, lds, s, g, bias, o);
  } else {
    if (band_lds) ensure_lds_attr((const void*)k_gemm_mask<Small, T>, Small::LDS + band_lds_bytes<Small>());
    hipLaunchKernelGGL((k_gemm_mask<Small, T>), dim3(ntile), dim3(Small::NT), Small::LDS + band_lds, s, g, bias, o);
  }
  GM2_CHECK_LAUNCH();
}

template void launch_gemm_mask<float>(const GemmArgs<float>&, const float*, const MaskOut&, bool, hipStream_t);
template void launch_gemm_mask<bf16_t>(const GemmArgs<bf16_t>&, const float*, const MaskOut&, bool, hipStream_t);

#ifdef GM2_DEBUG
GM2_DBG_TAKE_FN(dbg_take_gemm_mask)
#endif

}  // namespace gm2

