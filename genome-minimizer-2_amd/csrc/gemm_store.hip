// The fp32-store GEMM family (gemm_core.hpp): epilogue 1, k_gemm_store, its launchers and the plan
// queries that go with them.
#include "gemm_launch.hpp"

namespace gm2 {

namespace {

// ---------------------------------------------------------------------------------------------
// Epilogue 1: fp32 store. Rows m < msplit go to C0, rows >= msplit to C1 (row m - msplit); the
// split-K slice z writes slab z (C0 + z*slab). Optional per-column bias.
// ---------------------------------------------------------------------------------------------
//
// Optional BatchNorm statistics of the stored tile (bn.mode != 0; 128-row tiles, one K pass, no
// row split -- the host checks): per (128-row chunk = row tile, column) partials in the format of
// k_bn_fwd_partial / k_bn_bwd_partial, so the separate statistics pass over Y / dA disappears.
//   mode 1 (forward): v = acc + bias -> (chunk mean, M2), from sums of v - shift in fp32 with the
//           shift = the tile's first row (stable: the shift is a sample of the column).
//   mode 2 (backward): acc = dA; do = dA * [y*alpha + beta' > 0] with y read from bn.Y ->
//           (sum do, sum (y - mean) do).
// The store loop visits 4 fixed columns per thread, so the sums stay in registers and the threads
// of a column are combined through LDS once at the end.
__device__ __forceinline__ double sq4(float a, float b, float c, float d) {
  return ((double)a * a + (double)b * b) + ((double)c * c + (double)d * d);
}

// stamp 3 of the probes (gemm_core.hpp): the tile's stores acknowledged
__device__ __forceinline__ void stamp_end() {
#ifdef GM2_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  GM2_STAMP(3);
#endif
}

template <int EPI, int BM>
inline constexpr bool kRowEpi = BM == 128 && (EPI == 1 || EPI == 3 || EPI == 4);

// combine the threads of a column through LDS and write the tile's BatchNorm partials (mode 1 / 2)
template <class C>
__device__ __forceinline__ void stats_tail(int bmode, const TileXY tl, int M, int N, int n, const float (&sa)[4],
                                           const float (&sb)[4], const float (&sh)[4], const StoreEpi& bn,
                                           char* smem) {
  constexpr int TPR = C::BN / 4, RPI = C::NT / TPR;
  float4* red = (float4*)smem;
  red[2 * threadIdx.x] = make_float4(sa[0], sa[1], sa[2], sa[3]);
  red[2 * threadIdx.x + 1] = make_float4(sb[0], sb[1], sb[2], sb[3]);
  __syncthreads();
  if (threadIdx.x < TPR && n < N) {
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), q = a;
#pragma unroll
    for (int k = 0; k < RPI; ++k) {
      const float4 x = red[2 * (threadIdx.x + k * TPR)], y = red[2 * (threadIdx.x + k * TPR) + 1];
      a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
      q.x += y.x; q.y += y.y; q.z += y.z; q.w += y.w;
    }
    const float av[4] = {a.x, a.y, a.z, a.w}, qv[4] = {q.x, q.y, q.z, q.w};
    float2* o = bn.part + (int64_t)(tl.m0 / C::BM) * bn.ldp + n;
    const float nr = (float)min(C::BM, M - tl.m0);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (bmode == 1) {
        const float dm = av[u] / nr;
        o[u] = make_float2(sh[u] + dm, fmaxf(fmaf(-av[u], dm, qv[u]), 0.f));
      } else {
        o[u] = make_float2(av[u], qv[u]);
      }
    }
  }
}

// fixed-order block sum of the threads' sums of squares, one fp64 per tile (bn.sq; one K pass)
template <class C>
__device__ __forceinline__ void sq_tail(double sqa, const TileXY tl, int Np, const StoreEpi& bn, char* smem) {
  double* red = (double*)smem;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const double w = wave_sum_d(sqa);
  __syncthreads();
  if (lane == 0) red[wid] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < C::NT / 64; ++k) t += red[k];
    bn.sq[(tl.m0 / C::BM) * (Np / C::BN) + tl.n0 / C::BN] = t;
  }
}

// The per-column operands of the row-store kinds: loaded before the main loop, used after it.
struct RowCols {
  float bb[4], mean[4], alpha[4], beta[4];
};

template <int EPI>
__device__ __forceinline__ RowCols load_row_cols(int n, const float* __restrict__ bias, const StoreEpi& bn) {
  RowCols cc;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    cc.bb[u] = (EPI == 3 && bias) ? bias[n + u] : 0.f;
    cc.mean[u] = cc.alpha[u] = cc.beta[u] = 0.f;
    if constexpr (EPI == 4) {
      cc.mean[u] = bn.save[n + u];
      cc.alpha[u] = bn.save[bn.H + n + u] * bn.gamma[n + u];
      cc.beta[u] = fmaf(-cc.mean[u], cc.alpha[u], bn.beta[n + u]);
    }
  }
  return cc;
}

// The row-store epilogues of the 128x128 tiles (EPI 1 / 3 / 4; host-checked: 16-B aligned rows, one
// destination, N = Np). Same staging, values and summation order as the general code in store_tile
// (per thread rows ascending within a band, bands ascending), but no trip to memory is waited for
// between row passes: the passes are unrolled with rows past M predicated, a band's row stores go
// out back to back, and mode 2's Y rows are all requested before the accumulators are staged, so
// they land behind the staging and its barrier.
template <class C, int EPI>
__device__ __forceinline__ void store_rows(const TileXY tl, int M, int Np, float* __restrict__ Cz, int64_t ldc,
                                           const StoreEpi& bn, const RowCols& cc, const f32x4 (&acc)[C::FM][C::FN],
                                           char* smem) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wm = wid / C::WGN, wn = wid % C::WGN;
  float* img = (float*)smem;
  constexpr int pitch = C::BN + 4;
  constexpr int BR = 64, NBANDS = C::BM / BR, BPW = C::WTM / BR;
  constexpr int TPR = C::BN / 4, RPI = C::NT / TPR, NPASS = BR / RPI;
  static_assert(BR * pitch * 4 <= C::LDS && C::NT % TPR == 0 && BR % RPI == 0 && 2 * C::NT * 16 <= C::LDS,
                "epilogue shape");
  const int cq = (threadIdx.x % TPR) * 4, rq = threadIdx.x / TPR;
  const int n = tl.n0 + cq;
  // mode 2: the thread's Y rows, requested before the staging -- all bands' at once where that is
  // at most 8 float4 (the 8-wave tile), else band by band (the 4-wave tile: 8 per band)
  constexpr bool YALL = NBANDS * NPASS <= 8;
  float4 yv[NBANDS * NPASS];
  auto load_y = [&](int h) {  // (rows past M: the last valid row's address, value unused)
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int m = min(tl.m0 + h * BR + rq + p * RPI, M - 1);
      yv[h * NPASS + p] = *(const float4*)(bn.Y + (int64_t)m * bn.ldy + n);
    }
  };
  if constexpr (EPI == 4 && YALL) {
#pragma unroll
    for (int h = 0; h < NBANDS; ++h) load_y(h);
  }
  float sa[4] = {0.f, 0.f, 0.f, 0.f}, sb[4] = {0.f, 0.f, 0.f, 0.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
  double sqa = 0.0;
  // the bands of a tile with all BM rows valid (FULL: no predicate, so no branch around a store and
  // the compiler's vmcnt for a Y row counts exactly the loads and stores issued after it) or not
  auto bands = [&](auto full) {
    constexpr bool FULL = decltype(full)::value;
#pragma unroll
    for (int h = 0; h < NBANDS; ++h) {
      if constexpr (EPI == 4 && !YALL) load_y(h);
      if (wm == h / BPW) {
        const int mi0 = (h % BPW) * (BR / 16);
#pragma unroll
        for (int mi = 0; mi < BR / 16; ++mi)
#pragma unroll
          for (int ni = 0; ni < C::FN; ++ni)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              img[(mi * 16 + 4 * (lane >> 4) + j) * pitch + wn * C::WTN + ni * 16 + (lane & 15)] = acc[mi0 + mi][ni][j];
      }
      __syncthreads();
      if (EPI == 3 && h == 0) {  // shift = the tile's first row (always < M)
#pragma unroll
        for (int u = 0; u < 4; ++u) sh[u] = img[cq + u] + cc.bb[u];
      }
      float v[NPASS][4];
#pragma unroll
      for (int p = 0; p < NPASS; ++p) {
        const float4 w = *(const float4*)(img + (rq + p * RPI) * pitch + cq);
        v[p][0] = w.x + cc.bb[0], v[p][1] = w.y + cc.bb[1], v[p][2] = w.z + cc.bb[2], v[p][3] = w.w + cc.bb[3];
      }
#pragma unroll
      for (int p = 0; p < NPASS; ++p) {
        const int m = tl.m0 + h * BR + rq + p * RPI;
        if (FULL || m < M) *(float4*)(Cz + (int64_t)m * ldc + n) = make_float4(v[p][0], v[p][1], v[p][2], v[p][3]);
      }
#pragma unroll
      for (int p = 0; p < NPASS; ++p) {
        const bool ok = FULL || tl.m0 + h * BR + rq + p * RPI < M;
        if constexpr (EPI == 1) {
          const double q = sq4(v[p][0], v[p][1], v[p][2], v[p][3]);
          sqa = ok ? sqa + q : sqa;
        } else if constexpr (EPI == 3) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float dv = v[p][u] - sh[u];
            sa[u] = ok ? sa[u] + dv : sa[u];
            sb[u] = ok ? fmaf(dv, dv, sb[u]) : sb[u];
          }
        } else {
          const float4 y4 = yv[h * NPASS + p];
          float y[4] = {y4.x, y4.y, y4.z, y4.w};
          // (ties the row's sign tests to its image read: hoisted to where Y lands, the masks of
          // every row sat in SGPRs at once and spilled on the 4-wave tile)
          asm volatile("" : "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]) : "v"(v[p][0]));
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float d = fmaf(y[u], cc.alpha[u], cc.beta[u]) > 0.f ? v[p][u] : 0.f;
            sa[u] = ok ? sa[u] + d : sa[u];
            sb[u] = ok ? fmaf(y[u] - cc.mean[u], d, sb[u]) : sb[u];
          }
        }
      }
      __syncthreads();
    }
  };
  if (tl.m0 + C::BM <= M) bands(std::true_type{});
  else bands(std::false_type{});
  if constexpr (EPI != 1) stats_tail<C>(EPI == 3 ? 1 : 2, tl, M, Np, n, sa, sb, sh, bn, smem);
  if constexpr (EPI == 1) {
    if (bn.sq) sq_tail<C>(sqa, tl, Np, bn, smem);
  }
}

template <class C, typename T, bool AK, bool BK, bool PP, int IDX, int EPI, bool S3>
__device__ __forceinline__ void store_tile(const TileXY tl, const GemmArgs<T>& g, float* __restrict__ C0,
                                           float* __restrict__ C1, int msplit, int64_t ldc, int64_t slab,
                                           const float* __restrict__ bias, const StoreEpi& bn, char* smem);

// IDX (zero-copy rows, PP only): 1 = P's rows through g.prow, 2 = Q's k-rows through g.qrow; the
// tile's slice of the index array sits in an LDS table after the staging ring
// EPI (the epilogue, fixed at compile time for the 256x256 kernels so each instantiation carries only
// its own store code: with the general one every 256x256 kernel spilled 12-21 VGPRs, with these
// none): 0 = general (bias, BatchNorm statistics, row split, unaligned rows, transposed store),
// 1 = plain fp32 store (split-K slabs or one pass, rows aligned or not, optional per-tile sums of
// squares), 2 = the transposed store through the LDS image (+ sums of squares)
// The 128x128 kernels take the row-store kinds (store_rows below: aligned whole rows, no row split,
// no N edge; store_epi picks them on the host): 1 = plain or split-K slab store (+ sums of squares),
// 3 = optional bias + forward BatchNorm statistics (mode 1), 4 = backward statistics (mode 2);
// 0 stays the fallback for everything else
// S3 (PP only; GM2_BF16X3 training): both operands in the split layout of k_split_kmajor / k_split_rows
// (g.K = twice the real K) and the main loop in its hi.hi + hi.lo + lo.hi form
template <class C, typename T, bool AK, bool BK, bool PP, int IDX = 0, int EPI = 0, bool S3 = false>
__global__ __launch_bounds__(C::NT, C::MINW) void k_gemm_store(GemmArgs<T> g, float* __restrict__ C0, float* __restrict__ C1,
                                                    int msplit, int64_t ldc, int64_t slab,
                                                    const float* __restrict__ bias, StoreEpi bn) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  GM2_STAMP(0);
  const int tm = g.Mp / C::BM, tn = g.Np / C::BN;
  if (bn.ntiles == 0) {  // one tile per workgroup
    store_tile<C, T, AK, BK, PP, IDX, EPI, S3>(tile_of<C>(tm, tn), g, C0, C1, msplit, ldc, slab, bias, bn, smem);
    return;
  }
  // capped grid (one K pass): workgroup wg takes logical tiles wg, wg + grid, ... (every wave of
  // the block runs the same trip count; the LDS is reused after a barrier)
  const int ntile = tm * tn;
  for (int t = xcd_wg(); t < bn.ntiles; t += gridDim.x) {
    __syncthreads();
    store_tile<C, T, AK, BK, PP, IDX, EPI, S3>(tile_at<C>(t % ntile, tm, tn, t / ntile), g, C0, C1, msplit, ldc, slab,
                                               bias, bn, smem);
  }
}

template <class C, typename T, bool AK, bool BK, bool PP, int IDX, int EPI, bool S3>
__device__ __forceinline__ void store_tile(const TileXY tl, const GemmArgs<T>& g, float* __restrict__ C0,
                                           float* __restrict__ C1, int msplit, int64_t ldc, int64_t slab,
                                           const float* __restrict__ bias_in, const StoreEpi& bn, char* smem) {
  // (the specialised epilogues: their options fixed, so the general code below folds away)
  const float* __restrict__ bias = EPI == 0 ? bias_in : nullptr;
  const int bmode = EPI == 0 ? bn.mode : 0;
  const int btrans = EPI == 0 ? bn.trans : EPI == 2;
  const int kbeg = tl.split * g.k_per_split;
  const int kend = min(g.K, kbeg + g.k_per_split);
  const int nk = (kend - kbeg) / E<T>::KT;
  GM2_DBG(tl.m0 + C::BM <= g.Mp && tl.n0 + C::BN <= g.Np && kbeg >= 0 && kend <= g.K, kDbgTile);
  f32x4 acc[C::FM][C::FN];
  RowCols cols;
  if constexpr (kRowEpi<EPI, C::BM>) cols = load_row_cols<EPI>(tl.n0 + (threadIdx.x % (C::BN / 4)) * 4, bias_in, bn);
  if constexpr (PP) {
    int* sidx = (int*)(smem + C::LDS);
    if constexpr (IDX == 1) {
      for (int i = threadIdx.x; i < C::BM; i += C::NT) {
        sidx[i] = g.prow[tl.m0 + i];
        GM2_DBG(sidx[i] >= 0 && (g.idx_lim == 0 || sidx[i] < g.idx_lim), kDbgGemmIdx);
      }
      __syncthreads();
    } else if constexpr (IDX == 2) {
      for (int i = threadIdx.x; i < kend - kbeg; i += C::NT) {
        sidx[i] = g.qrow[kbeg + i];
        GM2_DBG(sidx[i] >= 0 && (g.idx_lim == 0 || sidx[i] < g.idx_lim), kDbgGemmIdx);
      }
      __syncthreads();
    }
    mainloop_pp<AK, BK, IDX, S3>(g.P, g.ldp, g.Q, g.ldq, tl.m0, tl.n0, kbeg, nk, smem, acc, sidx);
  } else {
    static_assert(IDX == 0 && !S3, "zero-copy rows, split operands: ping-pong main loop only");
    mainloop<C, T, AK, BK>(g.P, g.ldp, g.Q, g.ldq, tl.m0, tl.n0, kbeg, nk, smem, acc);
  }
  GM2_STAMP(2);
  float* Cz = C0 + (int64_t)tl.split * slab;
  if constexpr (kRowEpi<EPI, C::BM>) {
    store_rows<C, EPI>(tl, g.M, g.Np, Cz, ldc, bn, cols, acc, smem);
    stamp_end();
    return;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wm = wid / C::WGN, wn = wid % C::WGN;
  // Stage one 64-row band of the tile at a time through the (now free) staging LDS (row pitch
  // BN + 4 floats: the accumulator writes of lanes 16 apart land 16 banks apart), then store whole
  // rows with 16-byte stores (4 columns per thread; scalar where C's rows are not 16-B aligned or
  // at the N edge).
  // Transposed store (btrans): 16 lanes write 4 consecutive m each of one column n (256
  // contiguous bytes of C^T's row n), reading the image down a column (odd pitch: conflict-free).
  float* img = (float*)smem;
  const int pitch = btrans ? C::BN + 1 : C::BN + 4;
  constexpr int BR = 64, NBANDS = C::BM / BR, BPW = C::WTM / BR;  // bands, bands per wave row
  static_assert(BR * (C::BN + 4) * 4 <= C::LDS, "epilogue band must fit the staging LDS");
  constexpr int TPR = C::BN / 4, RPI = C::NT / TPR;  // threads per row, rows per pass
  static_assert(C::NT % TPR == 0 && BR % RPI == 0 && 2 * C::NT * 16 <= C::LDS, "epilogue shape");
  const int cq = (threadIdx.x % TPR) * 4, rq = threadIdx.x / TPR;
  const int n = tl.n0 + cq;
  const bool vec = ((ldc | slab) & 3) == 0 && ((((uintptr_t)C0) | ((uintptr_t)C1)) & 15) == 0;
  // Rows that are not 16-B aligned (ldc % 4 != 0, e.g. the [H][G] input-layer gradient at odd G):
  // row m's elements go into the image shifted by e_m = (address of (m, n0) in floats) % 4, so
  // every image chunk of 4 is one aligned 16-B global chunk; only the two end chunks of a row are
  // partial. e_m depends on the row only through m % 4 (j of the accumulator layout).
  const bool shiftvec = !vec && slab == 0 && !bias && bmode == 0 && !btrans && msplit >= g.M &&
                        (((uintptr_t)C0) & 3) == 0;
  const int e_base = (int)(((uintptr_t)(C0 + (int64_t)tl.m0 * ldc + tl.n0) >> 2) & 3), l3 = (int)(ldc & 3);
  float bb[4], sa[4], sb[4], sh[4], bmean[4], balpha[4], bbeta[4];
  double sqa = 0.0;  // sum of squares of the stored values (bn.sq), fp64 like the re-reading pass
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    bb[u] = (bias && n + u < g.N) ? bias[n + u] : 0.f;
    sa[u] = sb[u] = sh[u] = bmean[u] = balpha[u] = bbeta[u] = 0.f;
    if (bmode == 2 && n + u < g.N) {
      bmean[u] = bn.save[n + u];
      balpha[u] = bn.save[bn.H + n + u] * bn.gamma[n + u];
      bbeta[u] = fmaf(-bmean[u], balpha[u], bn.beta[n + u]);
    }
  }
#pragma unroll
  for (int h = 0; h < NBANDS; ++h) {
    if (wm == h / BPW) {
      const int mi0 = (h % BPW) * (BR / 16);
#pragma unroll
      for (int mi = 0; mi < BR / 16; ++mi)
#pragma unroll
        for (int ni = 0; ni < C::FN; ++ni)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            img[(mi * 16 + 4 * (lane >> 4) + j) * pitch + wn * C::WTN + ni * 16 + (lane & 15) +
                (shiftvec ? (e_base + j * l3) & 3 : 0)] = acc[mi0 + mi][ni][j];
    }
    __syncthreads();
    if (btrans) {
      const int q = threadIdx.x & 15;
      const int m = tl.m0 + h * BR + 4 * q;
      for (int c = threadIdx.x >> 4; c < C::BN; c += C::NT / 16) {
        const int nn = tl.n0 + c;
        if (nn >= g.N || m >= g.M) continue;
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = img[(4 * q + u) * pitch + c];
        float* dst = C0 + (int64_t)nn * ldc + m;
        if (vec && m + 3 < g.M) {
          *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
          sqa += sq4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (m + u < g.M) {
              dst[u] = v[u];
              sqa += (double)v[u] * v[u];
            }
        }
      }
      __syncthreads();
      continue;
    }
    if (h == 0 && bmode == 1) {  // shift = the tile's first row (always < M)
#pragma unroll
      for (int u = 0; u < 4; ++u) sh[u] = img[cq + u] + bb[u];
    }
    for (int r = rq; r < BR; r += RPI) {
      const int m = tl.m0 + h * BR + r;
      if (m >= g.M) break;
      if (shiftvec) {
        const int e = (e_base + r * l3) & 3;  // image position p holds column p - e
        float* rowp = C0 + (int64_t)m * ldc + tl.n0 - e;  // rowp + p: 16-B aligned for p % 4 == 0
        const float4 w = *(const float4*)(img + r * pitch + cq);
        const int c0 = cq - e;
        if (c0 >= 0 && tl.n0 + c0 + 3 < g.N) {
          *(float4*)(rowp + cq) = w;
          sqa += sq4(w.x, w.y, w.z, w.w);
        } else {
          const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (c0 + u >= 0 && tl.n0 + c0 + u < g.N) {
              rowp[cq + u] = wv[u];
              sqa += (double)wv[u] * wv[u];
            }
        }
        if (cq == 0 && e > 0) {  // the end chunk: positions BN .. BN + e - 1
          const float4 t = *(const float4*)(img + r * pitch + C::BN);
          const float tv[4] = {t.x, t.y, t.z, t.w};
          for (int u = 0; u < e; ++u)
            if (tl.n0 + C::BN - e + u < g.N) {
              rowp[C::BN + u] = tv[u];
              sqa += (double)tv[u] * tv[u];
            }
        }
        continue;
      }
      const float4 w = *(const float4*)(img + r * pitch + cq);
      const float v[4] = {w.x + bb[0], w.y + bb[1], w.z + bb[2], w.w + bb[3]};
      float* dst = (EPI != 0 || m < msplit ? Cz + (int64_t)m * ldc : C1 + (int64_t)(m - msplit) * ldc) + n;
      if (vec && n + 3 < g.N) {
        *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
        sqa += sq4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (n + u < g.N) {
            dst[u] = v[u];
            sqa += (double)v[u] * v[u];
          }
      }
      if (bmode == 1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float dv = v[u] - sh[u];
          sa[u] += dv;
          sb[u] = fmaf(dv, dv, sb[u]);
        }
      } else if (bmode == 2) {
        const float4 y4 = *(const float4*)(bn.Y + (int64_t)m * bn.ldy + n);
        const float y[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float d = fmaf(y[u], balpha[u], bbeta[u]) > 0.f ? v[u] : 0.f;
          sa[u] += d;
          sb[u] = fmaf(y[u] - bmean[u], d, sb[u]);
        }
      }
    }
    __syncthreads();
  }
  // (the two tails below: stats_tail and sq_tail spelt out -- calling the helpers here cost the
  // 256x256 zero-copy kernel a spilled register)
  if (bmode) {  // (bn mode: N % 4 == 0, one K pass, 128-row tiles -- checked on the host)
    float4* red = (float4*)smem;
    red[2 * threadIdx.x] = make_float4(sa[0], sa[1], sa[2], sa[3]);
    red[2 * threadIdx.x + 1] = make_float4(sb[0], sb[1], sb[2], sb[3]);
    __syncthreads();
    if (threadIdx.x < TPR && n < g.N) {
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), q = a;
#pragma unroll
      for (int k = 0; k < RPI; ++k) {
        const float4 x = red[2 * (threadIdx.x + k * TPR)], y = red[2 * (threadIdx.x + k * TPR) + 1];
        a.x += x.x; a.y += x.y; a.z += x.z; a.w += x.w;
        q.x += y.x; q.y += y.y; q.z += y.z; q.w += y.w;
      }
      const float av[4] = {a.x, a.y, a.z, a.w}, qv[4] = {q.x, q.y, q.z, q.w};
      float2* o = bn.part + (int64_t)(tl.m0 / C::BM) * bn.ldp + n;
      const float nr = (float)min(C::BM, g.M - tl.m0);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (bmode == 1) {
          const float dm = av[u] / nr;
          o[u] = make_float2(sh[u] + dm, fmaxf(fmaf(-av[u], dm, qv[u]), 0.f));
        } else {
          o[u] = make_float2(av[u], qv[u]);
        }
      }
    }
  }
  if (bn.sq) {  // (one K pass: checked on the host) fixed-order block sum, one fp64 per tile
    double* red = (double*)smem;
    const double w = wave_sum_d(sqa);
    __syncthreads();
    if (lane == 0) red[wid] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < C::NT / 64; ++k) t += red[k];
      bn.sq[(tl.m0 / C::BM) * (g.Np / C::BN) + tl.n0 / C::BN] = t;
    }
  }
  stamp_end();
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
// the tile / split-K plan (gemm_plan.hpp) under the call's GM2_OPT_SMALL_SPLIT
template <typename T>
GemmPlan plan_gemm(const GemmArgs<T>& g) {
  return plan_gemm_dims((int)sizeof(T), g.Mp, g.Np, g.K, opts().small_split);
}

template <typename T>
static bool use_big(const GemmArgs<T>& g) {
  return plan_gemm(g).tile == 256;
}

// where an fp32-store launch writes: rows m < msplit to C0, the rest to C1 (null: all to C0), row
// pitch ldc, split-K slice z at offset z * slab; bias added when non-null
struct StoreOut {
  float* C0;
  float* C1;
  int msplit;
  int64_t ldc, slab;
  const float* bias;
};

template <class C, typename T, bool AK, bool BK, bool PP, int IDX = 0, int EPI = 0, bool S3 = false>
static void store_launch_k(const GemmArgs<T>& a, int tiles, const StoreOut& o, const StoreEpi& bn, hipStream_t s) {
  // (zero-copy rows: the index table after the staging ring -- a tile's rows, or a split's k-rows)
  constexpr int table_max = IDX == 1 ? C::BM * 4 : IDX == 2 ? kMaxIdxRows * 4 : 0;
  static_assert(C::LDS + table_max <= 160 * 1024, "LDS budget");
  const int lds = C::LDS + (IDX == 1 ? C::BM * 4 : IDX == 2 ? a.k_per_split * 4 : 0);
  if (lds > C::LDS + table_max) throw Gm2Error("gemm: %d bytes of LDS", lds);
  StoreEpi ep = bn;
  GridCap gc{tiles, 0};
  if (bn.ntiles) gc = capped_grid(tiles, device_cus());  // the same number of rounds on fewer CUs
  ep.ntiles = gc.ntiles;
  launch_lds(k_gemm_store<C, T, AK, BK, PP, IDX, EPI, S3>, gc.grid, C::NT, C::LDS + table_max, lds, s, a, o.C0,
             o.C1 ? o.C1 : o.C0, o.C1 ? o.msplit : (1 << 30), o.ldc, o.slab, o.bias, ep);
}

// the specialised epilogue a 256x256 launch can take (k_gemm_store EPI): 1 = plain fp32 store,
// 2 = transposed through LDS, 0 = general. A 128x128 launch (tile 128) takes a row-store kind where
// the rows are 16-B aligned, go to one destination and the tile columns end at N: 1 = plain or slab
// store, 3 = forward statistics (with or without bias), 4 = backward statistics; else 0
template <typename T>
static int store_epi(const GemmArgs<T>& a, const StoreOut& o, const StoreEpi& bn, int tile) {
  const bool aligned = ((o.ldc | o.slab) & 3) == 0 && (((uintptr_t)o.C0) & 15) == 0;
  const bool split = o.C1 && o.msplit < a.M;
  if (tile == 128) {
    if (!aligned || split || bn.trans || a.N != a.Np) return 0;
    if (bn.mode == 0) return o.bias ? 0 : 1;
    if (bn.sq) return 0;
    if (bn.mode == 1) return 3;
    return o.bias || bn.ldy % 4 || (((uintptr_t)bn.Y) & 15) ? 0 : 4;
  }
  if (o.bias || bn.mode || split) return 0;
  if (bn.trans) return aligned ? 2 : 0;
  return 1;
}

template <class C, typename T, bool AK, bool BK, bool PP, int IDX>
static void store_launch_epi(const GemmArgs<T>& a, int tiles, const StoreOut& o, const StoreEpi& bn, hipStream_t s) {
  switch (store_epi(a, o, bn, 256)) {
    case 1: return store_launch_k<C, T, AK, BK, PP, IDX, 1>(a, tiles, o, bn, s);
    case 2:  // (launch_gemm_trans's one caller, the output-layer weight gradient, has no row table)
      if constexpr (IDX == 0) return store_launch_k<C, T, AK, BK, PP, 0, 2>(a, tiles, o, bn, s);
      throw Gm2Error("zero-copy rows: transposed store not instantiated");
    default: return store_launch_k<C, T, AK, BK, PP, IDX, 0>(a, tiles, o, bn, s);
  }
}

// main loop, row table and epilogue of one fp32-store launch. s3 (GM2_BF16X3, 256x256 ping-pong
// tiles, plain fp32 store): three products per K-tile over split operands in the three layouts; with
// g.qrow (both MN-major) plain K-tiles, Q's k-rows through the row table
template <class C, typename T, bool AK, bool BK>
static void store_launch(const GemmArgs<T>& a, int tiles, const StoreOut& o, const StoreEpi& bn, bool s3,
                         hipStream_t s) {
  if constexpr (std::is_same_v<C, Big> && sizeof(T) == 2) {
    if (s3) {  // (launch_gemm_store_x3 has checked the ping-pong main loop is on)
      if (a.prow) throw Gm2Error("bf16x3 GEMM: P row table not instantiated");
      if (!a.qrow) return store_launch_k<C, T, AK, BK, true, 0, 1, true>(a, tiles, o, bn, s);
      if constexpr (!AK && !BK) return store_launch_k<C, T, false, false, true, 2, 1, false>(a, tiles, o, bn, s);
      throw Gm2Error("bf16x3 GEMM: row table with this layout not instantiated");
    }
    if (a.prow || a.qrow) {  // zero-copy rows: the input layer's two GEMMs (gemm_idx_ok checked)
      if (!pp_enabled()) throw Gm2Error("zero-copy rows need the ping-pong main loop");
      if constexpr (AK && BK) {
        if (a.prow && !a.qrow) return store_launch_epi<C, T, AK, BK, true, 1>(a, tiles, o, bn, s);
      }
      if constexpr (AK && !BK) {
        if (a.qrow && !a.prow) return store_launch_epi<C, T, AK, BK, true, 2>(a, tiles, o, bn, s);
      }
      throw Gm2Error("zero-copy rows: layout not instantiated");
    }
    if (pp_enabled()) return store_launch_epi<C, T, AK, BK, true, 0>(a, tiles, o, bn, s);
  }
  if (s3) throw Gm2Error("bf16x3 GEMM: bf16 256x256 tiles only");
  if (a.prow || a.qrow) throw Gm2Error("zero-copy rows: bf16 256x256 tiles only");
  if constexpr (C::BM == 128) {
    switch (store_epi(a, o, bn, 128)) {
      case 1: return store_launch_k<C, T, AK, BK, false, 0, 1>(a, tiles, o, bn, s);
      case 3: return store_launch_k<C, T, AK, BK, false, 0, 3>(a, tiles, o, bn, s);
      case 4: return store_launch_k<C, T, AK, BK, false, 0, 4>(a, tiles, o, bn, s);
      default: break;
    }
  }
  store_launch_k<C, T, AK, BK, false>(a, tiles, o, bn, s);
}

// one launch over the K-slices `splits` asks for (k_slices); returns the slices (= slabs) taken
template <class C, typename T>
static int store_impl(const GemmArgs<T>& g, int splits, const StoreOut& o, const StoreEpi& bn, bool s3, hipStream_t s) {
  GemmArgs<T> a = g;
  const KSlices ks = k_slices(g.K, E<T>::KT, splits);
  if (g.qrow && !row_table_fits(g.K, E<T>::KT, splits))
    throw Gm2Error("zero-copy rows: %d k-rows per split", ks.k_per_split);
  if (bn.sq && ks.splits != 1) throw Gm2Error("gemm: sums of squares need one K pass");
  a.k_per_split = ks.k_per_split;
  const int tiles = (g.Mp / C::BM) * (g.Np / C::BN) * ks.splits;
  TimedLaunch tl(kKcGemmStore, s);
  if (g.pk && g.qk) store_launch<C, T, true, true>(a, tiles, o, bn, s3, s);
  else if (g.pk && !g.qk) store_launch<C, T, true, false>(a, tiles, o, bn, s3, s);
  else if (!g.pk && !g.qk) store_launch<C, T, false, false>(a, tiles, o, bn, s3, s);
  else throw Gm2Error("gemm: layout (P MN-major, Q K-major) not instantiated");
  GM2_CHECK_LAUNCH();
  return ks.splits;
}

// the big-or-small dispatch of every fp32-store launcher: 256x256 tiles (bf16 only, see
// plan_gemm_dims) when `big`, else the 128x128 configuration the options select
template <typename T>
static int store_dispatch(const GemmArgs<T>& g, bool big, int splits, const StoreOut& o, const StoreEpi& ep, bool s3,
                          hipStream_t s) {
  if constexpr (sizeof(T) == 2) {
    if (big) {
      check_gemm(g, 256);
      return store_impl<Big, T>(g, splits, o, ep, s3, s);
    }
  }
  check_gemm(g, 128);
  return small_cfg<T>([&](auto cfg) { return store_impl<decltype(cfg), T>(g, splits, o, ep, s3, s); });
}

template <typename T>
int launch_gemm_store(const GemmArgs<T>& g, int splits, float* C0, float* C1, int msplit, int64_t ldc, int64_t slab,
                      const float* bias, hipStream_t s) {
  if (splits < 0) splits = plan_gemm(g).splits;
  return store_dispatch(g, use_big(g), splits, {C0, C1, msplit, ldc, slab, bias}, StoreEpi{}, false, s);
}

template <typename T>
int gemm_tiles(const GemmArgs<T>& g) {
  return use_big(g) ? (g.Mp / Big::BM) * (g.Np / Big::BN) : (g.Mp / SmallDeep::BM) * (g.Np / SmallDeep::BN);
}

template <typename T>
bool launch_gemm_sq(const GemmArgs<T>& g, float* C, int64_t ldc, double* sq, hipStream_t s, bool force_big) {
  // force_big: a one-pass 256x256-tile launch even where the plan would pick 128 tiles (a row
  // slice of a big-tile GEMM, same per-element results as the whole)
  const bool big = force_big ? (sizeof(T) == 2 && g.Mp % 256 == 0 && g.Np % 256 == 0) : use_big(g);
  if (force_big ? !big : plan_gemm(g).splits != 1) return false;
  StoreEpi ep;
  ep.sq = sq;
  ep.ntiles = (grid_cap_bits() & 2) && !force_big;  // dWe0 bit (store_launch_k sets the count)
  store_dispatch(g, big, 1, {C, nullptr, 0, ldc, 0, nullptr}, ep, false, s);
  return true;
}

template <typename T>
bool launch_gemm_trans(const GemmArgs<T>& g, float* C, int64_t ldc, hipStream_t s, double* sq) {
  if (plan_gemm(g).splits != 1) return false;
  StoreEpi ep;
  ep.trans = 1;
  ep.sq = sq;
  ep.ntiles = grid_cap_bits() & 1;  // dW9 bit (store_launch_k sets the count)
  store_dispatch(g, use_big(g), 1, {C, nullptr, 0, ldc, 0, nullptr}, ep, false, s);
  return true;
}

// BatchNorm statistics in the store epilogue (GM2_OPT_BN_EPILOGUE, default on): taken when the
// plan is one pass of 128-row tiles (the statistics chunk), else the caller runs the separate pass
template <typename T>
bool launch_gemm_bn(const GemmArgs<T>& g, float* C, int64_t ldc, const float* bias, const StoreEpi& bn, hipStream_t s) {
  static_assert(Small::BM == kBnRowChunk, "statistics chunk = row tile");
  if (!opts().bn_epilogue) return false;
  const GemmPlan p = plan_gemm(g);
  if (p.tile != 128 || p.splits != 1 || (bn.mode && (g.N % 4 || bn.ldy % 4))) return false;
  store_dispatch(g, false, 1, {C, nullptr, 0, ldc, 0, bias}, bn, false, s);
  return true;
}

// ---- GM2_BF16X3: the split-operand GEMMs (gm2_kernels.hpp) ----
template <typename T>
bool gemm_idx_ok(const GemmArgs<T>& g) {
  if (sizeof(T) != 2 || !pp_enabled()) return false;
  const GemmPlan p = plan_gemm<T>(g);
  // (P rows: one 256-row table per tile; Q k-rows: a K-slice's k-rows in the table)
  return p.tile == 256 && (!g.qrow || row_table_fits(g.K, E<T>::KT, p.splits));
}

bool gemm_x3_ok(const GemmArgs<bf16_t>& g) {
  return g.Mp % 256 == 0 && g.Np % 256 == 0 && g.K % 64 == 0 && gemm_idx_ok<bf16_t>(g);
}

int launch_gemm_store_x3(const GemmArgs<bf16_t>& g, int splits, float* C, int64_t ldc, int64_t slab, double* sq,
                         hipStream_t s) {
  if (!pp_enabled()) throw Gm2Error("bf16x3 GEMM needs the ping-pong main loop (GM2_OPT_GEMM_PP)");
  StoreEpi ep;
  ep.sq = sq;
  return store_dispatch(g, true, splits, {C, nullptr, 0, ldc, slab, nullptr}, ep, true, s);
}

#define GM2_INST(T)                                                                                              \
  template bool launch_gemm_trans<T>(const GemmArgs<T>&, float*, int64_t, hipStream_t, double*);                    \
  template bool launch_gemm_sq<T>(const GemmArgs<T>&, float*, int64_t, double*, hipStream_t, bool);                \
  template int gemm_tiles<T>(const GemmArgs<T>&);                        \
  template bool launch_gemm_bn<T>(const GemmArgs<T>&, float*, int64_t, const float*, const StoreEpi&, hipStream_t);   \
  template int launch_gemm_store<T>(const GemmArgs<T>&, int, float*, float*, int, int64_t, int64_t, const float*, \
                                    hipStream_t);                                                                \
  template GemmPlan plan_gemm<T>(const GemmArgs<T>&);                                                          \
  template bool gemm_idx_ok<T>(const GemmArgs<T>&);
GM2_INST(float)
GM2_INST(bf16_t)
#undef GM2_INST

#ifdef GM2_DEBUG
GM2_DBG_TAKE_FN(dbg_take_gemm_store)
#endif

}  // namespace gm2
