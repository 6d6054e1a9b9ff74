// The loss GEMM family (gemm_core.hpp): epilogue 2 in its two forms, k_gemm_recon_loss and
// k_gemm_recon_loss_x3, and their launchers.
#include "gemm_launch.hpp"

namespace gm2 {

namespace {

// ---------------------------------------------------------------------------------------------
// Epilogue 2: decoder output layer + reconstruction loss (loss_components.py:49-50 BCE(sum),
// :111-115 gene abundance) and, in training, dL/dlogit as autograd composes Sigmoid->BCE:
//   dp = (p-x)/max((1-p)p, 1e-12) + w*gamma ; dl = dp*(1-p)*p.
// (sign(colsum p) == 1 wherever p > 0, and dl == 0 wherever p == 0: no batch-wide pass needed.)
// The tile is computed TRANSPOSED: P = the output weight W9 [Gp][H] (rows = genes), Q = the last
// hidden activations A5 [Bp][H] (rows = strains), so acc holds logit^T and each lane owns FOUR
// CONSECUTIVE GENES of one strain row: 8-byte bf16 (16-byte f32) LDS image writes, one 32-bit word
// of the row-major target bits, a float4 of the bias.
// FAST (bf16 training path): hardware exp / rcp / log (~1 ulp), log(1-p) for log1p(-p), and the
// (p-x)/max(q,1e-12)*q product folded to (p-x) where q >= 1e-12 (the same value up to one
// rounding); the fp32 parity path keeps the reference's exact formula order.
// Writes dL [strain][ldd] (row-major, through an LDS image for full-line stores), zero outside the
// valid G x B box; per-tile BCE and sum(p) into loss_part[tile*2 + {0,1}]; per-(strain tile, gene)
// sums of dl into colpart (the output bias gradient).
// ---------------------------------------------------------------------------------------------
// The loss epilogue's element loop. No per-element guards: padded genes (g >= G) have a zero
// weight row and a zero bias, so their logit is exactly 0 and their BCE / sum(p) contributions are
// exact constants the kernel subtracts per tile; padded strains' sums are dropped per column. Padded dL entries are harmless: every consumer multiplies them by
// zero-padded operands (W9 shadow rows >= G, A5 rows >= B) or never reads them.
//
// FAST (bf16 training) element math, in the reference's own quantities: p = sigmoid(l) as
// rcp(1 + exp2(-l log2 e)) (hardware ~1 ulp), 1 - p formed in fp32 from p exactly as the reference
// forms it (so a p that rounds to 1.0 gives the reference's log(0) -> -100 clamp and zero gradient),
//   BCE = -max(log(x ? p : 1-p), -100)          (log(1-p) for log1p(-p): same value up to rounding)
//   dl  = (p - x) * min(p(1-p) * 1e12, 1) + w*gamma * p(1-p)
// which is the reference's ((p-x)/max(p(1-p),1e-12) + w*gamma) * (1-p) * p up to rounding. The
// selects are bit-field ops on a 0 / -1 mask from the target bit (x ? p : 1-p as |x ? p : p-1|,
// p - x as x ? p-1 : p), BCE is summed in log2 units and scaled by -ln 2 once per tile, and the
// bias arrives pre-scaled (nb = -b log2 e). BCE and sum(p) are summed per strain column and masked
// once per column (padded strains).
// Exact (fp32 parity) path: the reference's formula order, p computed first.
// Where fp32 sigmoid(l) is subnormal (l in about (-88.72, -87.34)), as observed on an MI355X
// (tests/test_gpu_loss_elements.py holds every path to bounds that contain both answers):
//   exact paths (k_gemm_recon_loss<Small, float>, k_gemm_recon_loss_x3): p stays subnormal as in the
//     reference, so a target of 1 gives BCE = |l| (87.5 .. 88.7) and dl = -p * 1e12 (~ -1e-26);
//   FAST path (bf16, 128 and 256 tile): p comes out 0 (probed at -87.5, -88, -88.5, -88.7; at -87.3,
//     where p is still normal, it is kept), so a target of 1 gives BCE = 100 (the clamp), dl = 0.
// From l = -89 down (exp overflows) every path and the reference give p = 0, BCE = 100, dl = 0.
// (m & a) | (~m & b) as one v_bfi_b32 (the compiler rewrites the C form into compare + select)
__device__ __forceinline__ float bfi(int m, float a, float b) {
  float r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
  return r;
}

// the exact element: (logit l, target bit x) -> BCE term and p added to bce / psum; returns dl
// (GRAD; else 0, and its arithmetic is gone)
struct ExactElem { float e, p, dl; };
template <bool GRAD>
__device__ __forceinline__ ExactElem recon_exact(float l, bool x, float wgam) {
  const float p = 1.0f / (1.0f + expf(-l));
  const float e = x ? -fmaxf(logf(p), -100.f) : -fmaxf(log1pf(-p), -100.f);
  if constexpr (!GRAD) return {e, p, 0.f};
  const float omp = 1.0f - p;
  const float dp = (p - (x ? 1.0f : 0.0f)) / fmaxf(omp * p, 1e-12f) + wgam;
  return {e, p, dp * omp * p};
}

template <class C, typename T, bool FAST, bool GRAD>
__device__ __forceinline__ void recon_tile(const f32x4 (&acc)[C::FM][C::FN], const uint32_t* __restrict__ xrow,
                                           int64_t ldxb, const float* bias_s, int N, int n0, int wm, int wn, int q,
                                           int c, float wgam, T* img, float& bce, float& psum,
                                           const int* xidx) {
  constexpr int PR = C::BM + 8;
  constexpr int XW = C::WTM / 32;  // target words of this wave's gene span per strain row
  static_assert(XW == 4 || XW == 2, "wave gene span");
  // strain-major order: one strain column (16 lanes x 4 genes x FM slices) at a time, so only
  // that strain's target words and one LDS row base are live (the image offsets of the FM slices
  // are immediates)
  // every strain column's target words are loaded up front (the main loop's fragment registers are
  // free now): one exposed load latency per tile instead of one per strain column
  uint32_t xwa[C::FN][XW];
#pragma unroll
  for (int ni = 0; ni < C::FN; ++ni) {
    const int sl = wn * C::WTN + ni * 16 + c;
    // (zero-copy rows: the strain's row of the resident target bits, from the tile's LDS table)
    const uint32_t* xp = xrow + (int64_t)(xidx ? xidx[sl] : n0 + sl) * ldxb;
    if (n0 + sl < N) {
      if constexpr (XW == 4) {
        const uint4 v = *(const uint4*)xp;
        xwa[ni][0] = v.x; xwa[ni][1] = v.y; xwa[ni][2] = v.z; xwa[ni][3] = v.w;
      } else {
        const uint2 v = *(const uint2*)xp;
        xwa[ni][0] = v.x; xwa[ni][1] = v.y;
      }
    } else {
#pragma unroll
      for (int k = 0; k < XW; ++k) xwa[ni][k] = 0u;
    }
  }
#pragma unroll
  for (int ni = 0; ni < C::FN; ++ni) {
    const int sl = wn * C::WTN + ni * 16 + c;  // strain (tile-local)
    const bool sok = n0 + sl < N;
    uint32_t xw[XW];
#pragma unroll
    for (int k = 0; k < XW; ++k) xw[k] = xwa[ni][k];
    // this lane's genes of word k sit at bits (mi & 1) * 16 + j after the shift by 4q
#pragma unroll
    for (int k = 0; k < XW; ++k) xw[k] >>= 4 * q;
    T* irow = img + sl * PR + wm * C::WTM + 4 * q;
    float bce_c = 0.f, ps_c = 0.f;
    f32x2_t bce2 = {0.f, 0.f}, ps2 = {0.f, 0.f};  // (FAST: pairs of elements)
    // the tile's bias slice sits in LDS (zero beyond G; pre-scaled by -log2 e on the FAST path);
    // slice mi + 1 is read while slice mi is computed
    const float* bsl = bias_s + wm * C::WTM + 4 * q;
    float4 b4n = *(const float4*)bsl;
#pragma unroll
    for (int mi = 0; mi < C::FM; ++mi) {
      const float4 b4 = b4n;
      if (mi + 1 < C::FM) b4n = *(const float4*)(bsl + (mi + 1) * 16);
      const float bn[4] = {b4.x, b4.y, b4.z, b4.w};
      float dl4[4];
      if constexpr (FAST) {
        // two elements per step in packed fp32 (v_pk_fma / v_pk_add / v_pk_mul: the register pairs
        // of the accumulator and the bias), the transcendentals, bit-field selects and clamps per
        // element; the same operations in the same order as one element at a time
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const f32x2_t a2 = {acc[mi][ni][2 * h], acc[mi][ni][2 * h + 1]};
          const f32x2_t b2 = {bn[2 * h], bn[2 * h + 1]};
          const f32x2_t y2 = a2 * f32x2_t{-1.4426950408889634f, -1.4426950408889634f} + b2;  // -l log2 e
          const f32x2_t d2 = f32x2_t{__builtin_amdgcn_exp2f(y2.x), __builtin_amdgcn_exp2f(y2.y)} + 1.0f;
          const f32x2_t p2 = {__builtin_amdgcn_rcpf(d2.x), __builtin_amdgcn_rcpf(d2.y)};
          const f32x2_t nomp2 = p2 - 1.0f;  // -(1 - p)
          const int msk0 = __builtin_amdgcn_sbfe((int)xw[mi >> 1], (mi & 1) * 16 + 2 * h, 1);  // x ? -1 : 0
          const int msk1 = __builtin_amdgcn_sbfe((int)xw[mi >> 1], (mi & 1) * 16 + 2 * h + 1, 1);
          const float l0 = fmaxf(__builtin_amdgcn_logf(fabsf(bfi(msk0, p2.x, nomp2.x))), -144.26950408889634f);
          const float l1 = fmaxf(__builtin_amdgcn_logf(fabsf(bfi(msk1, p2.y, nomp2.y))), -144.26950408889634f);
          bce2 += f32x2_t{l0, l1};  // max(log2, -100/ln 2)
          ps2 += p2;
          const f32x2_t r2 = {bfi(msk0, nomp2.x, p2.x), bfi(msk1, nomp2.y, p2.y)};  // p - x
          // -(1 - p) p once (packed); the 1e-12 guard factor is one multiply with the clamp
          // modifier per element, and the gene-abundance term reuses the product
          const f32x2_t t2 = nomp2 * p2;
          const f32x2_t s2 = {__builtin_amdgcn_fmed3f(t2.x * -1e12f, 0.0f, 1.0f),
                              __builtin_amdgcn_fmed3f(t2.y * -1e12f, 0.0f, 1.0f)};
          f32x2_t dl2 = r2 * s2;
          dl2 = f32x2_t{-wgam, -wgam} * t2 + dl2;
          dl4[2 * h] = dl2.x;
          dl4[2 * h + 1] = dl2.y;
        }
      } else {
        const uint32_t xb = xw[mi >> 1] >> ((mi & 1) * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j)
        {
          const ExactElem r = recon_exact<true>(acc[mi][ni][j] + bn[j], (xb >> j) & 1u, wgam);
          bce_c += r.e;
          ps_c += r.p;
          dl4[j] = r.dl;
        }
      }
      if constexpr (GRAD) {
        if constexpr (sizeof(T) == 2) {
          uint2 pk;
          pk.x = f2bf2(dl4[0], dl4[1]);
          pk.y = f2bf2(dl4[2], dl4[3]);
          *(uint2*)(irow + mi * 16) = pk;
        } else {
          *(f32x4*)(irow + mi * 16) = f32x4{dl4[0], dl4[1], dl4[2], dl4[3]};
        }
      }
    }
    if constexpr (FAST) {
      bce_c = bce2.x + bce2.y;
      ps_c = ps2.x + ps2.y;
    }
    if (sok) {
      bce += bce_c;
      psum += ps_c;
    }
  }
}

// BCE / sum(p) of one padded gene (logit exactly 0, target 0): p = 1/2, BCE = -log(1/2)
template <bool FAST>
__device__ __forceinline__ void recon_pad_const(float& e0, float& p0) {
  if constexpr (FAST) {  // the FAST element math at l = 0, x = 0
    const float p = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(0.f));
    e0 = -fmaxf(__builtin_amdgcn_logf(fabsf(p - 1.0f)), -144.26950408889634f) * 0.6931471805599453f;
    p0 = p;
  } else {
    p0 = 1.0f / (1.0f + expf(-0.f));
    e0 = -fmaxf(log1pf(-p0), -100.f);
  }
}

template <class C, typename T, bool PP, bool GRAD>
__device__ __forceinline__ void recon_loss_tile(const TileXY tl, const GemmArgs<T>& g, const float* __restrict__ bias,
                                                const uint32_t* __restrict__ xbits, int64_t ldxb,
                                                const float* __restrict__ scal, T* __restrict__ dL, int64_t ldd,
                                                float* __restrict__ loss_part, float* __restrict__ colpart,
                                                int64_t ldcol, char* smem, const int32_t* __restrict__ xrows);

// ntiles > 0: capped grid, workgroup wg takes tiles wg, wg + grid, ... (GM2_OPT_GRID_CAP bit 4)
template <class C, typename T, bool PP, bool GRAD>
__global__ __launch_bounds__(C::NT) void k_gemm_recon_loss(GemmArgs<T> g, const float* __restrict__ bias,
                                                         const uint32_t* __restrict__ xbits, int64_t ldxb,
                                                         int ntiles, const float* __restrict__ scal,
                                                         T* __restrict__ dL, int64_t ldd,
                                                         float* __restrict__ loss_part, float* __restrict__ colpart,
                                                         int64_t ldcol, const int32_t* __restrict__ xrows) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  GM2_STAMP(0);
  const int tm = g.Mp / C::BM, tn = g.Np / C::BN;
  if (ntiles == 0) {
    recon_loss_tile<C, T, PP, GRAD>(tile_of<C>(tm, tn), g, bias, xbits, ldxb, scal, dL, ldd, loss_part, colpart,
                                    ldcol, smem, xrows);
    return;
  }
  for (int t = xcd_wg(); t < ntiles; t += gridDim.x) {
    __syncthreads();
    recon_loss_tile<C, T, PP, GRAD>(tile_at<C>(t, tm, tn, 0), g, bias, xbits, ldxb, scal, dL, ldd, loss_part,
                                    colpart, ldcol, smem, xrows);
  }
}

template <class C, typename T, bool PP, bool GRAD>
__device__ __forceinline__ void recon_loss_tile(const TileXY tl, const GemmArgs<T>& g, const float* __restrict__ bias,
                                                const uint32_t* __restrict__ xbits, int64_t ldxb,
                                                const float* __restrict__ scal, T* __restrict__ dL, int64_t ldd,
                                                float* __restrict__ loss_part, float* __restrict__ colpart,
                                                int64_t ldcol, char* smem, const int32_t* __restrict__ xrows) {
  constexpr bool FAST = sizeof(T) == 2;
  // (m = genes, n = strains)
  // LDS: [0, image / staging) | per-row-group dl sums | BCE, sum(p) slots | bias slice
  constexpr int EPC = 16 / sizeof(T);
  constexpr int PR = C::BM + 8;
  constexpr int CPR = C::BM / EPC;      // 16-byte chunks per image row
  constexpr int RG = C::NT / CPR;       // row groups of the store pass
  constexpr int IMG = std::max<int>(C::LDS, C::BN * PR * (int)sizeof(T));
  float* colred = (float*)(smem + IMG);  // [RG][BM]
  float* red = colred + RG * C::BM;     // [2][32]
  float* bias_s = red + 64;             // [BM]
  int* xidx = (int*)(bias_s + C::BM);   // [BN] zero-copy strain rows of the target bits
  for (int i = threadIdx.x; i < C::BM; i += C::NT) {
    const float b = tl.m0 + i < g.M ? bias[tl.m0 + i] : 0.f;
    bias_s[i] = FAST ? b * -1.4426950408889634f : b;
  }
  if (xrows)
    for (int i = threadIdx.x; i < C::BN; i += C::NT) {
      xidx[i] = xrows[tl.n0 + i];
      GM2_DBG(xidx[i] >= 0 && (g.idx_lim == 0 || xidx[i] < g.idx_lim), kDbgReconRows);
    }
  GM2_DBG(tl.m0 + C::BM <= g.Mp && tl.n0 + C::BN <= g.Np, kDbgTile);
  f32x4 acc[C::FM][C::FN];
  if constexpr (PP)
    mainloop_pp<true, true>(g.P, g.ldp, g.Q, g.ldq, tl.m0, tl.n0, 0, g.K / E<T>::KT, smem, acc);
  else
    mainloop<C, T, true, true>(g.P, g.ldp, g.Q, g.ldq, tl.m0, tl.n0, 0, g.K / E<T>::KT, smem, acc);
  GM2_STAMP(2);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wm = wid / C::WGN, wn = wid % C::WGN;
  const int q = lane >> 4, c = lane & 15;
  const float wgam = scal[kScalWGamma];
  float bce = 0.f, psum = 0.f;
  T* img = (T*)smem;  // LDS image [BN strains][BM genes + 8] of T
  // (one element loop with the gene-abundance FMA for every preset: at w*gamma = 0 it leaves dl bit
  // for bit as it was, costs half a packed FMA per element, and keeps the kernel to one copy of the
  // loop -- with a second, FMA-free copy behind a uniform branch it spilled 42 VGPRs, with one 4)
  recon_tile<C, T, FAST, GRAD>(acc, xbits + ((tl.m0 + wm * C::WTM) >> 5), ldxb, bias_s, g.N, tl.n0, wm, wn, q, c, wgam,
                               img, bce, psum, xrows ? xidx : nullptr);
  if constexpr (FAST) bce *= -0.6931471805599453f;
  GM2_STAMP(4);
  if constexpr (GRAD) {
    __syncthreads();
    // dL rows (strains) of BM genes: full 16-byte stores along each row. Thread i keeps one chunk
    // column (EPC genes) over rows i/CPR, +RG, ...: the same pass sums that chunk's dl over the
    // valid strains for the output bias gradient (the rounded values the dW9 GEMM reads).
    const int cch = threadIdx.x % CPR, r0 = threadIdx.x / CPR;
    float cs[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) cs[e] = 0.f;
    for (int r = r0; r < C::BN; r += RG) {
      const uint4 v = *(const uint4*)(img + r * PR + cch * EPC);
      // (non-temporal: the 451-MB dL stream does not displace the output-layer weights, which
      // the loss GEMM re-reads from the Infinity Cache across strain tiles)
      __builtin_nontemporal_store(u32x4_t{v.x, v.y, v.z, v.w},
                                  (u32x4_t*)(dL + (int64_t)(tl.n0 + r) * ldd + tl.m0 + cch * EPC));
      if (tl.n0 + r < g.N) {
        if constexpr (sizeof(T) == 2) {
          const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            cs[2 * e] += __uint_as_float(w[e] << 16);
            cs[2 * e + 1] += __uint_as_float(w[e] & 0xFFFF0000u);
          }
        } else {
          cs[0] += __uint_as_float(v.x); cs[1] += __uint_as_float(v.y);
          cs[2] += __uint_as_float(v.z); cs[3] += __uint_as_float(v.w);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < EPC; ++e) colred[r0 * C::BM + cch * EPC + e] = cs[e];
  }
  bce = wave_sum(bce);
  psum = wave_sum(psum);
  if (lane == 0) { red[wid] = bce; red[32 + wid] = psum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < C::NT / 64; ++w) { a += red[w]; b += red[32 + w]; }
    // padded genes of an edge tile: logit exactly 0 -> p = 1/2, x = 0, BCE = -log(1/2) each
    // (a tile may lie wholly in the padding when Gp - G >= BM: the bf16 workspaces pad G to 256)
    const int pad_g = min(C::BM, max(0, tl.m0 + C::BM - g.M)), val_s = min(C::BN, g.N - tl.n0);
    if (pad_g > 0) {
      float e0, p0;
      recon_pad_const<FAST>(e0, p0);
      a -= (float)pad_g * (float)val_s * e0;
      b -= (float)pad_g * (float)val_s * p0;
    }
    loss_part[tl.t * 2 + 0] = a;
    loss_part[tl.t * 2 + 1] = b;
  }
  if constexpr (GRAD) {
    for (int cc = threadIdx.x; cc < C::BM; cc += C::NT) {
      const int gg = tl.m0 + cc;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < RG; ++w) v += colred[w * C::BM + cc];
      if (gg < g.M) colpart[(int64_t)(tl.n0 / C::BN) * ldcol + gg] = v;
    }
  }
#ifdef GM2_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  GM2_STAMP(3);
#endif
}

template <class C, typename T>
constexpr int recon_lds_bytes() {
  constexpr int img = std::max<int>(C::LDS, C::BN * (C::BM + 8) * (int)sizeof(T));
  constexpr int rg = C::NT / (C::BM / (16 / (int)sizeof(T)));
  return img + (rg * C::BM + 64 + C::BM + C::BN) * 4;
}

// ---------------------------------------------------------------------------------------------
// Epilogue 2 for GM2_BF16X3: the loss epilogue in its exact (non-FAST) form behind the 256x256
// ping-pong main loop in its S3 form, over W9 and A5 in the split layout (g.K = 2H). dL, colpart and
// the loss partials are fp32 as in the GM2_F32 kernel. The exact element math on 128 accumulator
// registers per lane does not fit the 256 a wave of this tile has (it spilled 334), so the math
// moves out of the fragment layout: the raw logits go through an LDS image, and the pass that
// stores dL computes bias, sigmoid, BCE and dl for the 4 genes x 16 strains each thread owns, in a
// rolled loop. A 256-strain fp32 image would not fit the LDS, so the image holds 128 strains and is
// filled twice, each time from half of every wave's strain fragments (every wave works in both).
// The tile may reach past what the fp32 workspace allocates (its gene axis is padded to 128, its
// rows to the 128-padded batch): elements at genes >= gcols or strains >= drows are not touched.
// dL is zero outside the valid G x B box; padded genes and strains add nothing to the sums.
// ---------------------------------------------------------------------------------------------
constexpr int kX3ImgRows = 128;
constexpr int recon_x3_img_bytes() { return std::max<int>(Big::LDS, kX3ImgRows * (Big::BM + 8) * 4); }
constexpr int recon_x3_lds_bytes() { return recon_x3_img_bytes() + (8 * Big::BM + 64 + Big::BM) * 4; }

template <bool GRAD>
__device__ __forceinline__ void recon_loss_tile_x3(const TileXY tl, const GemmArgs<bf16_t>& g,
                                                   const float* __restrict__ bias, const uint32_t* __restrict__ xbits,
                                                   int64_t ldxb, const float* __restrict__ scal, float* __restrict__ dL,
                                                   int64_t ldd, int gcols, int drows, float* __restrict__ loss_part,
                                                   float* __restrict__ colpart, int64_t ldcol, char* smem) {
  using C = Big;
  constexpr int PR = C::BM + 8;
  constexpr int CPR = C::BM / 4;   // 16-byte chunks per image row
  constexpr int RG = C::NT / CPR;  // row groups of the element pass
  static_assert(RG == 8 && C::FN == 4 && C::WTN == 64 && C::FM == 8, "bf16x3 loss tile shape");
  float* colred = (float*)(smem + recon_x3_img_bytes());  // [RG][BM]
  float* red = colred + RG * C::BM;                       // [2][32]
  float* bias_s = red + 64;                               // [BM]
  GM2_DBG(tl.m0 + C::BM <= g.Mp && tl.n0 + C::BN <= g.Np, kDbgTile);
  f32x4 acc[C::FM][C::FN];
  mainloop_pp<true, true, 0, true>(g.P, g.ldp, g.Q, g.ldq, tl.m0, tl.n0, 0, g.K / 64, smem, acc);
  {
    // the tile's bias slice, filled after the main loop (read behind the first barrier below). The
    // index is made opaque so that its LDS address is formed here and not kept in a register -- a
    // spilled one -- across the main loop of every tile of a capped grid
    int i = threadIdx.x;
    asm volatile("" : "+v"(i));
    if (i < C::BM) bias_s[i] = tl.m0 + i < g.M ? bias[tl.m0 + i] : 0.f;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, wm = wid / C::WGN, wn = wid % C::WGN;
  const int q = lane >> 4, c = lane & 15;
  const float wgam = scal[kScalWGamma];
  float* img = (float*)smem;  // [128 strains][BM genes + 8] raw logits
  // the element pass: this thread's 4 genes (chunk cch) of image rows r0, r0 + RG, ...
  const int cch = threadIdx.x % CPR, r0 = threadIdx.x / CPR;
  const int gene0 = tl.m0 + cch * 4;
  const bool col_ok = gene0 < gcols;
  const uint32_t* xcol = xbits + (gene0 >> 5);
  const int xsh = gene0 & 31;
  float bce = 0.f, psum = 0.f;
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    // this half's logits: strain fragments 2h, 2h + 1 of every wave -> image row wn * 32 + (ni & 1) * 16 + c
#pragma unroll
    for (int nl = 0; nl < 2; ++nl) {
      float* irow = img + (wn * 32 + nl * 16 + c) * PR + wm * C::WTM + 4 * q;
#pragma unroll
      for (int mi = 0; mi < C::FM; ++mi) *(f32x4*)(irow + mi * 16) = acc[mi][2 * h + nl];
    }
    __syncthreads();
    if (col_ok) {
      const float4 b4 = *(const float4*)(bias_s + cch * 4);
      const float bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll 1
      for (int r = r0; r < kX3ImgRows; r += RG) {
        const int strain = tl.n0 + (r >> 5) * 64 + h * 32 + (r & 31);
        if (strain >= drows) continue;
        const bool sok = strain < g.N;
        float dl4[4] = {0.f, 0.f, 0.f, 0.f};
        if (sok) {
          const float4 v4 = *(const float4*)(img + r * PR + cch * 4);
          const float v[4] = {v4.x, v4.y, v4.z, v4.w};
          const uint32_t xw = xcol[(int64_t)strain * ldxb] >> xsh;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (gene0 + j >= g.M) continue;
            // (the reference's formula order, as the GM2_F32 kernel's exact path)
            const ExactElem r = recon_exact<GRAD>(v[j] + bs[j], (xw >> j) & 1u, wgam);
            bce += r.e;
            psum += r.p;
            dl4[j] = r.dl;
            if constexpr (GRAD) cs[j] += dl4[j];
          }
        }
        if constexpr (GRAD)
          __builtin_nontemporal_store(f32x4{dl4[0], dl4[1], dl4[2], dl4[3]},
                                      (f32x4*)(dL + (int64_t)strain * ldd + gene0));
      }
    }
    __syncthreads();  // (the image is rewritten by the second half)
  }
  if constexpr (GRAD) {
#pragma unroll
    for (int e = 0; e < 4; ++e) colred[r0 * C::BM + cch * 4 + e] = cs[e];
  }
  bce = wave_sum(bce);
  psum = wave_sum(psum);
  if (lane == 0) { red[wid] = bce; red[32 + wid] = psum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
    for (int w = 0; w < C::NT / 64; ++w) { a += red[w]; b += red[32 + w]; }
    loss_part[tl.t * 2 + 0] = a;
    loss_part[tl.t * 2 + 1] = b;
  }
  if constexpr (GRAD) {
    for (int cc = threadIdx.x; cc < C::BM; cc += C::NT) {
      const int gg = tl.m0 + cc;
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < RG; ++w) v += colred[w * C::BM + cc];
      if (gg < g.M) colpart[(int64_t)(tl.n0 / C::BN) * ldcol + gg] = v;
    }
  }
}

template <bool GRAD>
__global__ __launch_bounds__(Big::NT) void k_gemm_recon_loss_x3(GemmArgs<bf16_t> g, const float* __restrict__ bias,
                                                                const uint32_t* __restrict__ xbits, int64_t ldxb,
                                                                int ntiles, const float* __restrict__ scal,
                                                                float* __restrict__ dL, int64_t ldd, int gcols, int drows,
                                                                float* __restrict__ loss_part,
                                                                float* __restrict__ colpart, int64_t ldcol) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tm = g.Mp / Big::BM, tn = g.Np / Big::BN;
  if (ntiles == 0) {
    recon_loss_tile_x3<GRAD>(tile_of<Big>(tm, tn), g, bias, xbits, ldxb, scal, dL, ldd, gcols, drows, loss_part, colpart,
                             ldcol, smem);
    return;
  }
  for (int t = xcd_wg(); t < ntiles; t += gridDim.x) {
    __syncthreads();
    recon_loss_tile_x3<GRAD>(tile_at<Big>(t, tm, tn, 0), g, bias, xbits, ldxb, scal, dL, ldd, gcols, drows, loss_part,
                             colpart, ldcol, smem);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
// the loss GEMM's tile: 256x256 when it fills the chip (bf16 only: the fp32 parity path stays on the
// 128-tile, a 256-row fp32 dL image would not fit the LDS). GM2_OPT_RECON_TILE: 0 = plan,
// 128 / 256 = force (A/B measurements)
template <typename T>
static bool recon_big(const GemmArgs<T>& g) {
  const int force = opts().recon_tile;
  const bool ok = sizeof(T) == 2 && g.Mp % 256 == 0 && g.Np % 256 == 0;
  if (force == 128) return false;
  if (force == 256) return ok;
  return ok && (g.Mp / 256) * (g.Np / 256) >= 128;
}

template <typename T>
int gemm_recon_grid_blocks(const GemmArgs<T>& g) {
  const int t = recon_big(g) ? 256 : 128;
  return (g.Np / t) * (g.Mp / t);
}

template <typename T>
int gemm_recon_row_tiles(const GemmArgs<T>& g) {  // strain tiles (rows of colpart)
  return g.Np / (recon_big(g) ? 256 : 128);
}

template <typename T>
void launch_gemm_recon_loss(const GemmArgs<T>& g, const float* bias, const uint32_t* X, int64_t ldx, int with_grad,
                            const float* scal, T* dL, int64_t ldd, float* loss_part, float* colpart, int64_t ldcol,
                            hipStream_t s, const int32_t* xrows) {
  TimedLaunch tl(kKcReconLoss, s);
  // go(tile configuration, ping-pong main loop): the checks and the launch of that kernel
  auto go = [&](auto cfg, auto pp) {
    using C = decltype(cfg);
    constexpr bool PP = decltype(pp)::value;
    check_gemm(g, C::BM);
    if (ldx * 32 < g.Mp || (ldx & 3)) throw Gm2Error("recon: target bit rows too short");
    constexpr int lds = recon_lds_bytes<C, T>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    const GridCap gc = grid_for((g.Mp / C::BM) * (g.Np / C::BN), 4);
    auto kern = with_grad ? k_gemm_recon_loss<C, T, PP, true> : k_gemm_recon_loss<C, T, PP, false>;
    launch_lds(kern, gc.grid, C::NT, lds, lds, s, g, bias, X, ldx, gc.ntiles, scal, dL, ldd, loss_part, colpart, ldcol,
               xrows);
  };
  bool big = false;
  if constexpr (sizeof(T) == 2) {
    big = recon_big(g);
    if (big && pp_enabled()) go(Big{}, std::true_type{});
    else if (big) go(Big{}, std::false_type{});
  }
  if (!big) go(Small{}, std::false_type{});
  GM2_CHECK_LAUNCH();
}

bool gemm_recon_x3_ok(const GemmArgs<bf16_t>& g) { return pp_enabled() && g.K % 64 == 0 && recon_big<bf16_t>(g); }

void launch_gemm_recon_loss_x3(const GemmArgs<bf16_t>& g, const float* bias, const uint32_t* X, int64_t ldx,
                               int with_grad, const float* scal, float* dL, int64_t ldd, int gcols, int drows,
                               float* loss_part, float* colpart, int64_t ldcol, hipStream_t s) {
  TimedLaunch tl(kKcReconLoss, s);
  check_gemm(g, 256);
  if (gcols % 128 || gcols > ldd || ldx * 32 < gcols || (ldx & 3) || (ldd & 3) || (((uintptr_t)dL) & 15))
    throw Gm2Error("bf16x3 recon: gcols %d, ldd %lld, target pitch %lld", gcols, (long long)ldd, (long long)ldx);
  constexpr int lds = recon_x3_lds_bytes();
  static_assert(lds <= 160 * 1024, "LDS budget");
  const GridCap gc = grid_for((g.Mp / 256) * (g.Np / 256), 4);
  launch_lds(with_grad ? k_gemm_recon_loss_x3<true> : k_gemm_recon_loss_x3<false>, gc.grid, Big::NT, lds, lds, s, g,
             bias, X, ldx, gc.ntiles, scal, dL, ldd, gcols, drows, loss_part, colpart, ldcol);
  GM2_CHECK_LAUNCH();
}

#define GM2_INST(T)                                                                                              \
  template int gemm_recon_grid_blocks<T>(const GemmArgs<T>&);                                                   \
  template int gemm_recon_row_tiles<T>(const GemmArgs<T>&);                                                     \
  template void launch_gemm_recon_loss<T>(const GemmArgs<T>&, const float*, const uint32_t*, int64_t, int,        \
                                          const float*, T*, int64_t, float*, float*, int64_t, hipStream_t,      \
                                          const int32_t*);
GM2_INST(float)
GM2_INST(bf16_t)
#undef GM2_INST

#ifdef GM2_DEBUG
GM2_DBG_TAKE_FN(dbg_take_gemm_recon)
#endif

}  // namespace gm2
