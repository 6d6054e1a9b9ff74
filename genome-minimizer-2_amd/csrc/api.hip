// C-ABI of libgm2 (include/gm2.h): workspace layout + the per-step kernel schedule of the VAE
// train / eval / sample hot path. Host-side only; kernels live in gemm_*.hip and kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gm2.h"
#include "gm2_common.hpp"
#include "gm2_kernels.hpp"

using namespace gm2;

namespace {

thread_local std::string g_err;

#define HIP_OK(x)                                                                                  \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) throw Gm2Error("%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
  } while (0)

template <typename F>
int guarded(F&& f) {
  try {
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -1;
  } catch (...) {
    g_err = "unknown error";
    return -2;
  }
}

// reference parameter order (model.py:65-91)
enum P {
  E0W, E0B, E1G, E1BT, E3W, E3B, E4G, E4BT, E6W, E6B, E7G, E7BT, MUW, MUB, LVW, LVB,
  D0W, D0B, D1G, D1BT, D3W, D3B, D4G, D4BT, D6W, D6B, D7G, D7BT, D9W, D9B, NP
};
static_assert(NP == GM2_NUM_PARAMS, "param count");

struct Dims {
  int64_t G, H, L, Bm;
  int64_t Gp, Lp, K2L, L2r, Lr;
  int64_t off[NP + 1];
};

// gpad: the padding of the gene axis G. The bf16 workspaces pad it to 256 so that every GEMM with a
// G-wide side (input layer, output layer + loss, their weight gradients) tiles into the 256x256
// kernels (C5's G = 20,000 would otherwise be 20,096 = 78.5 x 256 and fall to the 128-tiles); the
// f32 workspaces (sampling decode, parity) keep 128.
Dims make_dims(const gm2_dims* d, int gpad = kTile) {
  if (!d) throw Gm2Error("null dims");
  Dims x;
  x.G = d->G, x.H = d->H, x.L = d->L;
  if (x.G <= 0 || x.H <= 0 || x.L <= 0 || d->batch_max <= 0) throw Gm2Error("dims must be positive");
  if (x.H % kTile) throw Gm2Error("hidden_dim %lld must be a multiple of 128", (long long)x.H);
  if (256 % x.L) throw Gm2Error("latent_dim %lld must divide 256", (long long)x.L);
  x.Bm = round_up(d->batch_max, kTile);
  x.Gp = round_up(x.G, gpad);
  x.Lp = round_up(x.L, kKPad);
  x.K2L = round_up(2 * x.L, kKPad);
  x.L2r = round_up(2 * x.L, kTile);
  x.Lr = round_up(x.Lp, kTile);
  const int64_t G = x.G, H = x.H, L = x.L;
  const int64_t sz[NP] = {H * G, H, H, H, H * H, H, H, H, H * H, H, H, H, L * H, L, L * H, L,
                          H * L, H, H, H, H * H, H, H, H, H * H, H, H, H, G * H, G};
  x.off[0] = 0;
  for (int i = 0; i < NP; ++i) x.off[i + 1] = x.off[i] + sz[i];
  return x;
}

// ---------------------------------------------------------------------------------------------
// workspace layout (bytes). Everything 256-B aligned. Element size es = 4 (F32) or 2 (BF16).
// ---------------------------------------------------------------------------------------------
// The gated sampling decode's control block (uint32 words, workspace region s3ctl):
//   [0, 16)    cumulative uint64[8] (k_decode_stats; zero from gm2_workspace_init), read by
//              gm2_workspace_stat: split tiles, exact tiles, band elements, band flips, band
//              overflow, decodes with split tiles, decodes without
//   [16, 48)   split-kernel tiles of this call (sharded), [48, 80) exact-kernel tiles
//   [80, 144)  band elements this call put in each list shard, 144 bits its recompute flipped
//   [160, 224) band elements this call put in tile slots (sharded)
//   [224, 256) single-product-kernel tiles of this call
//   [256, ...) block maxima of the row norms: activations (roundup(n, 256) / 256), then weights
// Words [16, 256 + blocks) are zeroed at the start of every gated decode.
struct DecodeCtl {
  static constexpr int kCum = 0, kTilesSplit = 16, kTilesExact = 48, kCounts = 80, kFlips = 80 + kBandShards,
                       kTileFound = 160, kTilesSingle = 160 + kBandShards, kBlk = kTilesSingle + kSplitShards;
  static_assert(kFlips < kTileFound && kBlk == 256, "control block");
};

struct Layout {
  Dims d;
  int prec;
  int64_t es;
  // GEMM shadows (T), natural [out][in] layout, zero-padded: each serves as a K-major operand in
  // the forward GEMM and as an MN-major operand ([K=out][N=in]) in the backward dX GEMM
  int64_t sE0, sE1, sE2, sHD, sD0, sD1, sD2, sD3;
  // the Linear weight of BatchNorm block i (kBlk)
  int64_t shadow(int i) const {
    const int64_t s[6] = {sE0, sE1, sE2, sD0, sD1, sD2};
    return s[i];
  }
  int64_t X, XB, Y[6], A[6], save[6], HD, Z, dL, slabs, slab_cap, side_slabs, side_cap, dY[6], DA, dH;
  int64_t AT5, dYT0;  // transposed A5 / dY0 [H][Bm]: K-major operands of the dW9 / dWe0 GEMMs
  int64_t bnpart, colpart, colpart_cap, losspart, losspart_cap, klpart, gradpart, clip, scal0, total;
  int64_t colbwd, colbwd_cap;  // per-layer bias-gradient partials of the backward (summed on the side stream)
  int64_t nahdr, nasq;         // norm-ahead header int[4] and per-tile sums of squares (NormAhead)
  int64_t X1, XB1;             // second input slot: the next batch's rows, staged under this step's tail
  int64_t syncb;               // SyncBN all-reduce vector: 2H + 2 doubles
  // gated sampling decode (f32 workspaces; GM2_OPT_SAMPLE_SPLIT): the split activations
  // [roundup(Bm, 256)][2H] and output weights [roundup(G, 256)][2H] (bf16, (hi | lo) per 32 columns),
  // their row norms (s3rn, s3cn), the control block (DecodeCtl), the band list and the split
  // kernel's per-tile band slots (s3tlist [tiles][kBandTileSlots] (row, gene), s3tcount [tiles])
  int64_t s3a, s3w, s3rn, s3cn, s3ctl, s3band, s3tlist, s3tcount;
  int64_t s3a1, s3w1;          // the single-product tier's operands: the hi parts alone, [rows][H] bf16
  // band-list overflow (MaskBand.oflag / olist / ocount, k_band_tile_fix), uint32 words: [0, 2) the
  // cumulative count of recomputed blocks (uint64), [4] this call's block count, [64, 64 + tiles) the
  // per-block flags, then [tiles] the listed block ids. Words [4, 64 + tiles) zeroed per decode.
  int64_t s3ovf;
  static constexpr int kOvfCount = 4, kOvfFlags = 64;
  // u8 masks of the gated decode (gm2_decode_mask): its packed bits [roundup(Bm, 256)][s3ldb], expanded
  // to the caller's rows by one streaming pass (k_expand_bits)
  int64_t s3bits, s3ldb;
  int64_t adamscal;            // scalar block of a queued output-layer Adam update
  int64_t ridx;                // zero-copy rows: int32 [roundup(Bm, 256)] resident-matrix row per batch row
  // GM2_BF16X3 (x3; otherwise empty regions): the split operands of the five G-wide GEMMs, bf16, with
  // Gq = roundup(G, 256), Bq = roundup(Bm, 256). K-major splits interleave (hi | lo) per 32 columns,
  // MN-major ones per 32 k-rows (launch_split_kmajor / launch_split_rows):
  //   x3w0  [H][2 Gq]   encoder.0.weight, K-major        x3xd  [Bq][2 Gq]  the 0/1 input rows as (x | x)
  //   x3w9k [Gq][2 H]   decoder.9.weight, K-major        x3x   [Bq][Gq]    the input rows once (dWe0's k-rows)
  //   x3w9m [2 Gq][H]   decoder.9.weight, MN-major       x3a5k [Bq][2 H], x3a5m [2 Bq][H]  last activations
  //   x3dlk [Bq][2 Gq], x3dlm [2 Bq][Gq]  dL             x3dy0 [2 Bq][H]   input layer's dY, MN-major
  //   x3rows int32 [2 Bq]: the row table that names every row of x3x twice (dWe0's exact side)
  bool x3 = false;
  int64_t Gq = 0, Bq = 0;
  int64_t x3w0, x3w9k, x3w9m, x3xd, x3x, x3a5k, x3a5m, x3dlk, x3dlm, x3dy0, x3rows;
};

// the control block (DecodeCtl) and the overflow area (Layout::s3ovf) of workspace `ws` by name, for a
// decode over Bq x Gq padded rows x genes (multiples of 256)
DecodeCounters decode_counters(char* ws, const Layout& l, int Bq, int Gq) {
  unsigned* ctl = (unsigned*)(ws + l.s3ctl);
  unsigned* ovf = (unsigned*)(ws + l.s3ovf);
  const int tiles = (Bq / 256) * (Gq / 256);
  DecodeCounters k;
  k.cum = (unsigned long long*)(ctl + DecodeCtl::kCum);
  k.ovf_cum = (unsigned long long*)ovf;
  k.tiles_split = ctl + DecodeCtl::kTilesSplit;
  k.tiles_exact = ctl + DecodeCtl::kTilesExact;
  k.tiles_single = ctl + DecodeCtl::kTilesSingle;
  k.shard_counts = ctl + DecodeCtl::kCounts;
  k.flips = ctl + DecodeCtl::kFlips;
  k.tile_found = ctl + DecodeCtl::kTileFound;
  k.ablk = ctl + DecodeCtl::kBlk;
  k.wblk = k.ablk + Bq / 256;
  k.ovf_count = ovf + Layout::kOvfCount;
  k.ovf_flags = ovf + Layout::kOvfFlags;
  k.ovf_list = k.ovf_flags + tiles;
  k.ctl_zero = k.tiles_split;
  k.ctl_zero_bytes = (size_t)(DecodeCtl::kBlk - DecodeCtl::kTilesSplit + Bq / 256 + Gq / 256) * 4;
  k.ovf_zero = k.ovf_count;
  k.ovf_zero_bytes = (size_t)(Layout::kOvfFlags - Layout::kOvfCount + tiles) * 4;
  return k;
}

#ifdef GM2_DEBUG
// (offset, bytes) of every region the last make_layout on this thread took (gm2_debug_check_layout)
thread_local std::vector<std::pair<int64_t, int64_t>> t_regions;
#endif

Layout make_layout(const gm2_dims* gd, int prec) {
  if (prec != GM2_F32 && prec != GM2_BF16 && prec != GM2_BF16X3) throw Gm2Error("bad precision %d", prec);
  Layout o;
  // (GM2_BF16X3: the GM2_F32 layout, then the split operand buffers)
  o.x3 = prec == GM2_BF16X3;
  if (o.x3) prec = GM2_F32;
  o.d = make_dims(gd, prec == GM2_BF16 ? 2 * kTile : kTile);
  o.prec = prec;
  o.es = prec == GM2_F32 ? 4 : 2;
  const Dims& d = o.d;
  int64_t cur = 0;
#ifdef GM2_DEBUG
  t_regions.clear();
#endif
  auto take = [&](int64_t bytes) {
    const int64_t at = cur;
    if (bytes < 0) throw Gm2Error("layout: negative region (%lld bytes)", (long long)bytes);
    cur += round_up(bytes, 256);
#ifdef GM2_DEBUG
    t_regions.emplace_back(at, bytes);
#endif
    return at;
  };
  const int64_t es = o.es, H = d.H, Bm = d.Bm;
  o.sE0 = take(H * d.Gp * es);       // [H][Gp]
  o.sE1 = take(H * H * es);          // [H][H]
  o.sE2 = take(H * H * es);
  o.sHD = take(d.L2r * H * es);      // [L2r][H]: rows 0..L-1 mean_layer, L..2L-1 logvar_layer
  o.sD0 = take(H * d.Lr * es);       // [H][Lr]
  o.sD1 = take(H * H * es);
  o.sD2 = take(H * H * es);
  o.sD3 = take(d.Gp * H * es);       // [Gp][H]
  o.X = take(Bm * d.Gp * es);        // gathered strain rows [Bm][Gp]
  o.XB = take(Bm * (d.Gp / 32) * 4); // row-major bit-packed target [Bm][Gp/32]
  for (int i = 0; i < 6; ++i) {
    o.Y[i] = take(Bm * H * 4);       // pre-BN fp32
    o.A[i] = take(Bm * H * es);      // post-ReLU
    o.save[i] = take(2 * H * 4);     // batch mean / invstd
  }
  o.HD = take(Bm * 2 * d.L * 4);     // mu | logvar fp32
  o.Z = take(Bm * d.Lr * es);        // z [Bm][Lr]
  o.dL = take(Bm * d.Gp * es);       // dL/dlogit [Bm][Gp]
  const int64_t maxN = std::max<int64_t>({H, 2 * d.L, d.Lr, 128});
  o.slab_cap = std::max<int64_t>(1024LL * kTile * kTile, 4 * Bm * maxN);
  o.slabs = take(o.slab_cap * 4);
  // weight-gradient GEMMs run on a side stream: their own split-K scratch, one dY per layer
  o.side_cap = std::max<int64_t>(8LL * H * std::max<int64_t>(H, d.L2r), 1024LL * kTile * kTile);
  o.side_slabs = take(o.side_cap * 4);
  for (int i = 0; i < 6; ++i) o.dY[i] = take(Bm * H * es);
  o.DA = take(Bm * H * 4);           // summed split-K input gradient (fp32)
  o.dH = take(Bm * d.L2r * es);      // d(mu | logvar) [Bm][L2r]
  o.AT5 = take(H * Bm * es);
  o.dYT0 = take(H * Bm * es);
  o.bnpart = take((Bm / kBnRowChunk) * H * 8);
  o.colpart_cap = std::max<int64_t>({(Bm / 64) * d.Gp, (Bm / 64) * H, (Bm / 64) * 2 * d.L});
  o.colpart = take(o.colpart_cap * 4);
  o.losspart_cap = std::max<int64_t>((d.Gp / kTile) * (Bm / kTile) * 2, Bm / 64);
  o.losspart = take(o.losspart_cap * 4);
  o.klpart = take((Bm / kReparamRows) * 4);
  o.gradpart = take(2048 * 2 * 8);
  o.colbwd_cap = std::max<int64_t>((Bm / 64) * std::max<int64_t>(H, 2 * d.L), (Bm / kReparamRows) * 2 * d.L);
  o.colbwd = take(7 * o.colbwd_cap * 4);
  o.nahdr = take(16);
  o.nasq = take(2 * (d.Gp / kTile + 1) * (H / kTile + 1) * 8);
  o.clip = take(64);
  o.scal0 = take(GM2_NUM_SCALARS * 4);
  o.X1 = take(Bm * d.Gp * es);
  o.XB1 = take(Bm * (d.Gp / 32) * 4);
  o.syncb = take((2 * H + 2) * 8);
  const bool split3 = prec == GM2_F32;
  o.s3a = take(split3 ? round_up(Bm, 2 * kTile) * 2 * H * 2 : 0);
  o.s3w = take(split3 ? round_up(d.G, 2 * kTile) * 2 * H * 2 : 0);
  o.s3rn = take(split3 ? round_up(Bm, 2 * kTile) * 4 : 0);
  o.s3cn = take(split3 ? round_up(d.G, 2 * kTile) * 4 : 0);
  o.s3ctl = take(split3 ? (DecodeCtl::kBlk + round_up(Bm, 2 * kTile) / 256 + round_up(d.G, 2 * kTile) / 256) * 4 : 0);
  o.s3band = take(split3 ? (int64_t)kBandShards * kBandShardCap * 8 : 0);
  const int64_t s3tiles = split3 ? (round_up(Bm, 2 * kTile) / 256) * (round_up(d.G, 2 * kTile) / 256) : 0;
  o.s3tlist = take(s3tiles * kBandTileSlots * 8);
  o.s3tcount = take(s3tiles * 4);
  o.s3a1 = take(split3 ? round_up(Bm, 2 * kTile) * H * 2 : 0);
  o.s3w1 = take(split3 ? round_up(d.G, 2 * kTile) * H * 2 : 0);
  o.s3ovf = take(split3 ? (Layout::kOvfFlags + 2 * s3tiles) * 4 : 0);
  o.s3ldb = split3 ? round_up(d.G, 2 * kTile) / 8 : 0;
  o.s3bits = take(split3 ? round_up(Bm, 2 * kTile) * o.s3ldb : 0);
  o.adamscal = take(GM2_NUM_SCALARS * 4);
  o.ridx = take(round_up(Bm, 2 * kTile) * 4);
  o.Gq = round_up(d.G, 2 * kTile);
  o.Bq = round_up(Bm, 2 * kTile);
  const int64_t x3e = o.x3 ? 2 : 0, Gq = o.Gq, Bq = o.Bq;  // bytes per element of the split buffers
  o.x3w0 = take(H * 2 * Gq * x3e);
  o.x3w9k = take(Gq * 2 * H * x3e);
  o.x3w9m = take(2 * Gq * H * x3e);
  o.x3xd = take(Bq * 2 * Gq * x3e);
  o.x3x = take(Bq * Gq * x3e);
  o.x3a5k = take(Bq * 2 * H * x3e);
  o.x3a5m = take(2 * Bq * H * x3e);
  o.x3dlk = take(Bq * 2 * Gq * x3e);
  o.x3dlm = take(2 * Bq * Gq * x3e);
  o.x3dy0 = take(2 * Bq * H * x3e);
  o.x3rows = take(2 * Bq * x3e * 2);
  o.total = cur;
  return o;
}

struct WsState;

// the one f32 / bf16 branch: f(T{}) with T the element type of a GM2_F32 / GM2_BF16 layout
// (Layout::prec; a GM2_BF16X3 workspace has the GM2_F32 layout)
template <typename F>
void by_precision(int prec, F&& f) {
  if (prec == GM2_F32) f(float{});
  else f(bf16_t{});
}

template <typename T>
struct Ctx {
  const Layout& lo;
  char* ws;
  hipStream_t s;
  const Dims& d;
  int64_t slab_off, slab_cap;  // split-K scratch of this stream
  int64_t xo, xbo;             // input slot of this call: gathered rows X [Bm][Gp] (T), target bits
  WsState& st;                 // host-side state of the workspace
  // zero-copy rows (gm2_batch.resident, training calls): the input layer's GEMMs and the loss
  // epilogue read the resident matrix's rows through ridx [roundup(Bm, 256)] instead of X / XB
  const int32_t* ridx = nullptr;
  const T* xres = nullptr;
  int64_t ld_xres = 0;
  const uint32_t* xbres = nullptr;
  int64_t ld_xbres = 0;
  int64_t res_rows = 0;  // rows of the resident operands (their zero row included): bounds of ridx
  bool x3 = false;       // GM2_BF16X3 with GM2_OPT_TRAIN_SPLIT on: the G-wide GEMMs as split-bf16 products
  bf16_t* h(int64_t off) const { return (bf16_t*)(ws + off); }
  Ctx(const Layout& l, void* w, void* strm, WsState& state)
      : lo(l), ws((char*)w), s((hipStream_t)strm), d(l.d), slab_off(l.slabs), slab_cap(l.slab_cap), xo(l.X),
        xbo(l.XB), st(state) {}
  Ctx side(hipStream_t strm) const {
    Ctx c(*this);
    c.s = strm;
    c.slab_off = lo.side_slabs;
    c.slab_cap = lo.side_cap;
    return c;
  }
  T* t(int64_t off) const { return (T*)(ws + off); }
  float* f(int64_t off) const { return (float*)(ws + off); }
};

// ---------------------------------------------------------------------------------------------
// Host-side state of one workspace (keyed by its device address; created by gm2_workspace_init,
// dropped by gm2_workspace_release). Nothing here is shared between workspaces: two models, or a
// training and a sampling workspace, in one process keep their own options, side stream, gradient
// bucket events and staged input slot. One workspace is used from one host thread at a time.
//
//  * side stream for the weight-gradient GEMMs (fork/join through events; capture-safe), created
//    on first use; GM2_OPT_SIDE_STREAM = 0 keeps everything on the caller's stream: the same
//    GEMMs with the same split-K counts into the same buffers (the side work keeps its own
//    scratch, BwdPass::w), without the fork / join events.
//  * gradient buckets (data-parallel exchange): ranges of the flat gradient buffer in the order the
//    backward finalises them, each with an event recorded when its last gradient is written
//    (gm2_grad_bucket_bounds / gm2_wait_grad_bucket)
//      0: decoder.9.weight, decoder.9.bias      (output layer: first off the backward)
//      1: encoder.0.bias .. decoder.7.bias      (every hidden / head / BN tensor)
//      2..5: encoder.0.weight row quarters      (input layer: the last weight-gradient GEMM)
//  * the input-slot stage of gm2_batch.next (SlotState below).
// ---------------------------------------------------------------------------------------------
// Per-workspace input-slot state. A training call whose batch carries `next` gathers next's rows
// into the other slot during its own tail; the following training call finds them there (same
// data / ld / rows / n) and starts straight at the input-layer GEMM. Every other call that uses an
// input slot first waits for a pending stage and drops it (it writes slot 0).
struct SlotState {
  bool staged = false;
  int slot = 0;  // slot of the staged batch
  const uint8_t* data = nullptr;
  int64_t ld = 0, n = 0, total = 0;
  const int32_t* rows = nullptr;
  int prec = -1;
};

// The schedule's environment knobs, for A/Bs (tools/ and profiles/ name them); read once per process.
//  GM2_EVENT_FENCE=system: events that only order this device's own streams (fork / join ring, staged
//    input slot, deferred update) release at system scope, as the gradient-bucket events always do (a
//    collective's peers may read the buffer). Default device scope: a system-scope release writes the
//    L2 back at every fork of the backward (measured ~7 us of idle main stream per fork).
//  GM2_FORK_HOLD (3): the first layer of the backward whose own fork is taken (6 = every layer forks).
//    The side work of the layers above it (5, 4, 3, the heads) would queue behind dW9 anyway: it goes
//    with the fork of layer 2 instead, one ordering event in place of five (-7..-11 us per step,
//    profiles/r03_fork_batch_ab.txt; holding layer 2 as well measured +15 us).
//  GM2_DW9_AT (2): the kernel of the backward's chain behind which dW9 starts (output_weight_grad).
//  GM2_TAIL_MAIN: the forward's tail launch stays on the caller's stream instead of going in front of
//    dW9 on the side stream (profiles/r03_fwd_tail_side_ab.txt).
struct SchedEnv {
  unsigned order_event_flags;
  int fork_hold, dw9_at;
  bool tail_main;
};
const SchedEnv& sched_env() {
  static const SchedEnv env = [] {
    const char *fence = std::getenv("GM2_EVENT_FENCE"), *hold = std::getenv("GM2_FORK_HOLD");
    const char* at = std::getenv("GM2_DW9_AT");
    const unsigned scope = fence && std::string(fence) == "system" ? 0u : (unsigned)hipEventReleaseToDevice;
    return SchedEnv{hipEventDisableTiming | scope, hold ? std::max(1, std::atoi(hold)) : 3,
                    at ? std::max(0, std::atoi(at)) : 2, std::getenv("GM2_TAIL_MAIN") != nullptr};
  }();
  return env;
}

struct WsState {
  Options opt;
  int dev = -1;
  hipStream_t side = nullptr;
  std::vector<hipEvent_t> ev;  // fork/join ring
  size_t next = 0;
  hipEvent_t bucket[GM2_GRAD_BUCKETS] = {};
  int bucket_ev[GM2_GRAD_BUCKETS] = {0, 1, 2, 3, 4, 5};  // the event that marks bucket b final
  bool recorded = false;  // a training backward has recorded the bucket events
  SlotState slot;
  hipEvent_t slot_done = nullptr;
  gm2_allreduce_fn coll = nullptr;  // SyncBN's all-reduce (gm2_workspace_set_collective)
  void* coll_user = nullptr;
  hipEvent_t adam9_done = nullptr;  // a deferred output-layer Adam update (GM2_OPT_DEFER_OUTPUT_ADAM)
  bool adam9_pending = false;       // launched on the side stream, not yet joined
  int cus = 0;                      // compute units of dev
  int64_t exact_decodes = 0;        // decodes the host sent to the exact-fp32 kernel alone (probs requests,
                                    // GM2_OPT_SAMPLE_SPLIT = 0, preconditions): GM2_STAT_EXACT_DECODES
  const unsigned long long* decode_cum = nullptr;  // the gated decodes' cumulative device counters (DecodeCtl)
  const unsigned long long* decode_ovf = nullptr;  // their cumulative count of overflow-recomputed blocks
  int64_t x3_split = 0, x3_exact = 0;  // GM2_TSTAT_*: G-wide GEMMs of a GM2_BF16X3 workspace run split / exact
  // the queued (not yet launched) output-layer update: launched by kick() beside the next training
  // call's hidden layers, or by join() on the joining stream
  struct QueuedAdam {
    bool queued = false;
    int prec = 0;
    TensorTable tt{};
    const float* g = nullptr;
    float *p = nullptr, *m = nullptr, *v = nullptr;
    const float *scal = nullptr, *clip = nullptr;
  } qadam;

  void create() {
    HIP_OK(hipGetDevice(&dev));
    HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    for (auto& e : bucket) HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&slot_done, sched_env().order_event_flags));
    HIP_OK(hipEventCreateWithFlags(&adam9_done, sched_env().order_event_flags));
  }
  void destroy() {
    if (side) (void)hipStreamDestroy(side);
    for (auto e : ev) (void)hipEventDestroy(e);
    for (auto e : bucket)
      if (e) (void)hipEventDestroy(e);
    if (slot_done) (void)hipEventDestroy(slot_done);
    if (adam9_done) (void)hipEventDestroy(adam9_done);
    side = nullptr;
    ev.clear();
  }
  // the side stream when GM2_OPT_SIDE_STREAM is on (created on first use), else nullptr
  hipStream_t side_stream() {
    if (!opt.side_stream) return nullptr;
    if (!side) {
      HIP_OK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
      if (ev.empty()) {
        ev.resize(64);
        for (auto& e : ev) HIP_OK(hipEventCreateWithFlags(&e, sched_env().order_event_flags));
      }
    }
    return side;
  }
  void launch_queued(hipStream_t s, int max_grid = 0) {
    QueuedAdam& q = qadam;
    by_precision(q.prec, [&](auto tag) {
      launch_adam_fused<decltype(tag)>(q.tt, q.g, q.p, q.m, q.v, q.scal, q.clip, s, max_grid);
    });
    q.queued = false;
  }
  // a training call's forward, after its input-layer GEMM: start the queued output-layer update on
  // the side stream (ordered after everything on `s` so far)
  void kick(hipStream_t s) {
    if (!qadam.queued) return;
    const hipStream_t sd = side_stream();
    if (!sd) {
      launch_queued(s);
      return;
    }
    order(s, sd);
    // a few workgroups per CU, looping over the blocks: room stays for the hidden layers' GEMM
    // workgroups (an uncapped grid fills every CU and serialises them behind it)
    launch_queued(sd, std::max(1, opt.defer_adam) * std::max(1, cus));
    HIP_OK(hipEventRecord(adam9_done, sd));
    adam9_pending = true;
  }
  // make `s` see a deferred output-layer update: a queued one is launched on `s`, a running one
  // waited for
  void join(hipStream_t s) {
    if (qadam.queued) launch_queued(s);
    if (adam9_pending) HIP_OK(hipStreamWaitEvent(s, adam9_done, 0));
    adam9_pending = false;
  }
  // SyncBN: SUM-all-reduce `count` doubles at device pointer `buf` across the ranks, on `s`
  void allreduce(double* buf, int64_t count, hipStream_t s) {
    if (!coll) throw Gm2Error("GM2_OPT_SYNC_BN needs a collective (gm2_workspace_set_collective)");
    const int rc = coll(buf, count, (void*)s, coll_user);
    if (rc != 0) throw Gm2Error("SyncBN all-reduce failed (%d)", rc);
  }
  // make `to` wait for everything enqueued on `from` so far
  void order(hipStream_t from, hipStream_t to) {
    hipEvent_t e = ev[next++ % ev.size()];
    HIP_OK(hipEventRecord(e, from));
    HIP_OK(hipStreamWaitEvent(to, e, 0));
  }
};

std::mutex& ws_mutex() {
  static std::mutex mu;
  return mu;
}
std::map<void*, std::unique_ptr<WsState>>& ws_map() {
  static std::map<void*, std::unique_ptr<WsState>> m;
  return m;
}

// the state of `ws`; a workspace that was never initialised through gm2_workspace_init (or was
// released) is an error
WsState& ws_state(void* ws) {
  std::lock_guard<std::mutex> lk(ws_mutex());
  auto it = ws_map().find(ws);
  if (it == ws_map().end()) throw Gm2Error("workspace %p is not initialised (gm2_workspace_init)", ws);
  return *it->second;
}

// (re)initialise the state of `ws`: process-default options, no stage, fresh events
WsState& ws_reset(void* ws) {
  std::lock_guard<std::mutex> lk(ws_mutex());
  auto& slot = ws_map()[ws];
  if (slot) slot->destroy();
  slot.reset(new WsState());
  slot->opt = default_options();
  slot->create();
  return *slot;
}

// true: a queued output-layer update was discarded (gm2_workspace_release then returns 1)
bool ws_release(void* ws) {
  std::lock_guard<std::mutex> lk(ws_mutex());
  auto it = ws_map().find(ws);
  if (it == ws_map().end()) return false;
  WsState& st = *it->second;
  const bool dropped = st.qadam.queued;
  // A still-QUEUED output-layer update is dropped, not launched: release can run at garbage-collection
  // time, after the parameter / moment buffers it would write were freed (callers join with
  // gm2_workspace_join before releasing, as gm2.h says; the Python host does). A RUNNING one is
  // waited for: it reads its scalar block from the workspace memory about to be freed.
  st.qadam.queued = false;
  if (st.adam9_pending) {  // (launched on the side stream)
    if (st.side) HIP_OK(hipStreamSynchronize(st.side));
    else HIP_OK(hipEventSynchronize(st.adam9_done));
    st.adam9_pending = false;
  }
  st.destroy();
  ws_map().erase(it);
  return dropped;
}

// first row of quarter q (0..4) of the input-layer weight gradient [H][G]
int64_t input_quarter_row(const Dims& d, int q) { return (d.H * q) / 4; }

void bucket_bounds(const Dims& d, int64_t* lh) {
  lh[0] = d.off[D9W], lh[1] = d.off[NP];
  lh[2] = d.off[E0B], lh[3] = d.off[D9W];
  for (int q = 0; q < 4; ++q) {
    lh[4 + 2 * q] = input_quarter_row(d, q) * d.G;
    lh[5 + 2 * q] = input_quarter_row(d, q + 1) * d.G;
  }
}

// one fp32-store launch of g: plain, or (s3, GM2_BF16X3 operands in the split layout) the bf16x3 launcher
template <typename U>
int gemm_store(const GemmArgs<U>& g, bool s3, int S, float* C0, float* C1, int msplit, int64_t ldc, int64_t slab,
               hipStream_t s) {
  if constexpr (sizeof(U) == 2) {
    if (s3) return launch_gemm_store_x3(g, S, C0, ldc, slab, nullptr, s);
  }
  if (s3) throw Gm2Error("bf16x3 GEMM: bf16 operands only");
  return launch_gemm_store<U>(g, S, C0, C1, msplit, ldc, slab, nullptr, s);
}

// GEMM into the stream's fp32 slab scratch (split-K slices summed by the consumer): the plan's
// split count, at most what the scratch holds. Returns #slabs.
template <class CtxT, typename U>
int gemm_to_slabs(const CtxT& c, const GemmArgs<U>& g, int64_t ldc, bool s3 = false) {
  const int64_t slab = slab_elems_padded(g.Mp, ldc);
  const int S = splits_into_slabs(plan_gemm<U>(g).splits, slab, c.slab_cap);
  return gemm_store<U>(g, s3, S, c.f(c.slab_off), nullptr, 0, ldc, slab, c.s);
}

// GEMM into C0/C1 (fp32, row split at msplit; s3: C0 only). Launches with too few tiles to fill the
// chip are split over K into slabs and summed by k_slab_sum (deterministic order).
template <class CtxT, typename U>
void gemm_to(const CtxT& c, const GemmArgs<U>& g, float* C0, float* C1, int msplit, int64_t ldc, bool s3 = false) {
  const int64_t slab = slab_elems_dense(g.M, g.N);
  int S = splits_into_c(plan_gemm<U>(g).splits, slab, c.slab_cap, s3);
  if (S <= 1) {
    gemm_store<U>(g, s3, 1, C0, C1, msplit, ldc, 0, c.s);
    return;
  }
  S = gemm_store<U>(g, s3, S, c.f(c.slab_off), nullptr, 0, g.N, slab, c.s);
  launch_slab_sum(c.f(c.slab_off), S, slab, g.M, g.N, C0, C1, C1 ? msplit : g.M, ldc, c.s);
}

// The two big weight-gradient GEMMs of the backward (output layer dW9, stored transposed; input
// layer dWe0). When both are one K pass (`direct`) their epilogues also write per-tile sums of
// squares, [sq9 | sq0] in the norm-ahead area, so gm2_grad_norm need not re-read 2 x H x G floats.
template <typename T>
struct BigGrads {
  GemmArgs<T> g9, g0;
  bool direct;
  int n9, n0;
};
// the input-layer weight gradient as four row-quarter launches (GM2_OPT_INPUT_CHUNKS = 4): only
// when each quarter is whole 256-row tiles of a one-pass plan, like the full launch
template <typename T>
bool input_chunked(const BigGrads<T>& r, int H) {
  if (opts().input_chunks != 4 || H % 1024) return false;
  const GemmPlan p = plan_gemm<T>(r.g0);
  return p.splits == 1 && p.tile == 256;
}

template <typename T>
BigGrads<T> big_grads(const Ctx<T>& c, int Bp) {
  const Layout& l = c.lo;
  const int H = (int)c.d.H, G = (int)c.d.G, Gp = (int)c.d.Gp;
  BigGrads<T> r{{c.t(l.AT5), Bp, c.t(l.dL), Gp, H, G, Bp, H, Gp, 0, 1, 0},
                {c.t(l.dYT0), Bp, c.t(c.xo), Gp, H, G, Bp, H, Gp, 0, 1, 0}, false, 0, 0};
  if (c.ridx) {  // zero-copy rows: X's rows are the resident matrix's, through ridx
    r.g0.Q = c.xres, r.g0.ldq = c.ld_xres;
    r.g0.qrow = c.ridx, r.g0.idx_lim = c.res_rows;
  }
  r.direct = plan_gemm<T>(r.g9).splits == 1 && plan_gemm<T>(r.g0).splits == 1;
  r.n9 = gemm_tiles<T>(r.g9);
  r.n0 = gemm_tiles<T>(r.g0);
  if ((int64_t)(r.n9 + r.n0) > 2 * (c.d.Gp / kTile + 1) * (c.d.H / kTile + 1)) r.direct = false;
  if (input_chunked(r, (int)c.d.H)) r.direct = false;  // the quarter launches take no clip statistics
  return r;
}

// the 6 BatchNorm blocks: (linear weight, linear bias, bn gamma, bn beta)
const int kBlk[6][4] = {{E0W, E0B, E1G, E1BT}, {E3W, E3B, E4G, E4BT}, {E6W, E6B, E7G, E7BT},
                        {D0W, D0B, D1G, D1BT}, {D3W, D3B, D4G, D4BT}, {D6W, D6B, D7G, D7BT}};

// ---------------------------------------------------------------------------------------------
// GM2_BF16X3: which of the five G-wide GEMMs of a call run as split-bf16 products, with their
// operands in the workspace's split buffers (Layout x3*). A GEMM splits when the hidden width tiles
// by 256 and the bf16 plan of its doubled-K shape is a 256x256 one (the loss GEMM: when the 256x256
// loss kernel fills the chip); the others run the exact-fp32 kernels as GM2_F32 does.
//   enc0  Y = X . W0^T        plain K-tiles over (x | x) and (hi | lo): x.hi + x.lo (X is 0/1: exact)
//   loss  logit^T = W9 . A5^T  three products, the exact BCE epilogue, fp32 dL
//   dA5   = dL . W9           dL K-major, W9 MN-major, three products
//   dW9   = dL^T . A5         both MN-major, three products, stored as decoder.9.weight's gradient
//   dWe0  = dY0^T . X         dY0 MN-major split, X's k-rows named twice by a row table: hi.x + lo.x
// ---------------------------------------------------------------------------------------------
struct X3Plan {
  bool enc0 = false, loss = false, da5 = false, dw9 = false, dwe0 = false;
  GemmArgs<bf16_t> g_enc0{}, g_loss{}, g_da5{}, g_dw9{}, g_dwe0{};
  int Bq = 0;
  int count() const { return (int)enc0 + (int)loss + (int)da5 + (int)dw9 + (int)dwe0; }
};

template <typename T>
X3Plan x3_plan(const Ctx<T>& c, int B) {
  X3Plan p;
  if (!c.x3 || sizeof(T) != 4) return p;
  const Layout& l = c.lo;
  const int H = (int)c.d.H, G = (int)c.d.G, Gq = (int)l.Gq, Bq = (int)round_up(B, 2 * kTile);
  p.Bq = Bq;
  if (H % (2 * kTile) || Bq > l.Bq) return p;
  p.g_enc0 = GemmArgs<bf16_t>{c.h(l.x3xd), 2 * Gq, c.h(l.x3w0), 2 * Gq, B, H, 2 * Gq, Bq, H, 0};
  p.g_loss = GemmArgs<bf16_t>{c.h(l.x3w9k), 2 * H, c.h(l.x3a5k), 2 * H, G, B, 2 * H, Gq, Bq, 0};
  p.g_da5 = GemmArgs<bf16_t>{c.h(l.x3dlk), 2 * Gq, c.h(l.x3w9m), H, B, H, 2 * Gq, Bq, H, 0, 1, 0};
  p.g_dw9 = GemmArgs<bf16_t>{c.h(l.x3dlm), Gq, c.h(l.x3a5m), H, G, H, 2 * Bq, Gq, H, 0, 0, 0};
  p.g_dwe0 = GemmArgs<bf16_t>{c.h(l.x3dy0), H, c.h(l.x3x), Gq, H, G, 2 * Bq, H, Gq, 0, 0, 0};
  p.g_dwe0.qrow = (const int32_t*)(c.ws + l.x3rows);
  p.g_dwe0.idx_lim = Bq;
  p.enc0 = gemm_x3_ok(p.g_enc0);
  p.loss = gemm_recon_x3_ok(p.g_loss);
  p.da5 = gemm_x3_ok(p.g_da5);
  p.dw9 = gemm_x3_ok(p.g_dw9);
  p.dwe0 = gemm_x3_ok(p.g_dwe0);
  if (p.dwe0) {  // (the slab-capped count, as gemm_to takes it: the slices the launch will really have)
    const GemmArgs<bf16_t>& g = p.g_dwe0;
    const int S = splits_into_c(plan_gemm<bf16_t>(g).splits, slab_elems_dense(g.M, g.N), c.lo.slab_cap, true);
    p.dwe0 = row_table_fits(g.K, 64, S);
  }
  return p;
}

// The plans of one call on B rows, computed once (after the call's input slot or zero-copy operands
// are set in c: big_grads reads them) and shared by its forward and backward
template <typename T>
struct StepPlan {
  X3Plan xp;
  BigGrads<T> bg;
  // this step's backward takes the clip statistics (NormAhead): both big weight gradients in one
  // pass with the tile sums in their epilogues (the split ones take none)
  bool norm_ahead;
};
template <typename T>
StepPlan<T> step_plan(const Ctx<T>& c, int B) {  // (host arithmetic only: safe before B is range-checked)
  StepPlan<T> p{x3_plan<T>(c, B), big_grads<T>(c, (int)round_up(B, kTile)), false};
  p.norm_ahead = p.bg.direct && !p.xp.dw9 && !p.xp.dwe0;
  return p;
}

// Tensor tables. kind 0: the 9 Linear weights with their natural-layout shadow (tile0 counts
// 64x64 tiles; fp32 -> shadow sync). kind 1: all 30 parameters in reference order, weights with
// their shadow (tile0 counts 4096-element blocks; fused Adam writes the shadow).
template <typename T>
TensorTable make_table(const Ctx<T>& c, int kind = 0) {
  const Dims& d = c.d;
  const Layout& l = c.lo;
  TensorTable tt{};
  auto tiles_of = [&](const TensorDesc& e) {
    return kind == 1 ? (e.rows * e.cols + 4095) / 4096 : ((e.rows + 63) / 64) * ((e.cols + 63) / 64);
  };
  auto add = [&](int pi, int64_t rows, int64_t cols, int64_t sh, int64_t sld, int64_t srow0) {
    TensorDesc& e = tt.t[tt.n];
    e.off = d.off[pi], e.rows = rows, e.cols = cols, e.shadowT = nullptr, e.tld = 0;
    e.shadow = sh >= 0 ? (void*)(c.ws + sh) : nullptr, e.sld = sld, e.srow0 = srow0;
    e.tile0 = tt.n == 0 ? 0 : tt.t[tt.n - 1].tile0 + tiles_of(tt.t[tt.n - 1]);
    tt.n++;
  };
  const int64_t H = d.H, G = d.G, L = d.L;
  auto vec = [&](int pi, int64_t n) {
    if (kind == 1) add(pi, 1, n, -1, 0, 0);
  };
  add(E0W, H, G, l.sE0, d.Gp, 0);
  vec(E0B, H); vec(E1G, H); vec(E1BT, H);
  add(E3W, H, H, l.sE1, H, 0);
  vec(E3B, H); vec(E4G, H); vec(E4BT, H);
  add(E6W, H, H, l.sE2, H, 0);
  vec(E6B, H); vec(E7G, H); vec(E7BT, H);
  add(MUW, L, H, l.sHD, H, 0);
  vec(MUB, L);
  add(LVW, L, H, l.sHD, H, L);
  vec(LVB, L);
  add(D0W, H, L, l.sD0, d.Lr, 0);
  vec(D0B, H); vec(D1G, H); vec(D1BT, H);
  add(D3W, H, H, l.sD1, H, 0);
  vec(D3B, H); vec(D4G, H); vec(D4BT, H);
  add(D6W, H, H, l.sD2, H, 0);
  vec(D6B, H); vec(D7G, H); vec(D7BT, H);
  add(D9W, G, H, l.sD3, H, 0);
  vec(D9B, G);
  return tt;
}

// the resident matrix rows of a batch: 16-B aligned rows of at least roundup(G, 128) bytes (gm2.h)
void check_batch_data(const gm2_batch* b, const Dims& d, const char* what) {
  if (!b->data) throw Gm2Error("%s: null data", what);
  if (b->ld_data % 16 || b->ld_data < round_up(d.G, kTile) || ((uintptr_t)b->data & 15))
    throw Gm2Error("%s: data rows must be 16-B aligned with ld_data (%lld) a multiple of 16 and >= roundup(G, 128)",
                   what, (long long)b->ld_data);
}

// entries [lo, hi) of a kind-1 table, block indices re-based to 0 (a launch over that subset)
TensorTable table_range(const TensorTable& tt, int lo, int hi) {
  TensorTable r{};
  const int64_t base = tt.t[lo].tile0;
  for (int i = lo; i < hi; ++i) {
    r.t[r.n] = tt.t[i];
    r.t[r.n].tile0 -= base;
    r.n++;
  }
  return r;
}

// ---------------------------------------------------------------------------------------------
// The forward schedule, written once: one Linear -> BatchNorm -> ReLU layer (bn_layer), the encoder
// half (rows, layers 0-2, heads + reparameterisation) and the decoder half (layers 3-5).
// ---------------------------------------------------------------------------------------------
// what the six BatchNorm layers of one pass share: parameters, running statistics [6][2H], rows
struct BnPass {
  const float* prm;
  float* bn;
  int B, Bp;
  int train = 0;      // batch statistics (Linear epilogue partials, running-statistics update)
  bool sync = false;  // SyncBN: the batch statistics span every rank's rows
  bool save = false;  // keep each layer's batch mean / invstd (Layout::save), as a backward needs
};

// Pre-BatchNorm Linear of layer i: Y_i = in . W_i^T + bias (fp32 [Bp][H]) and, when training, the
// per-128-row chunk (mean, M2) partials of Y_i -> bnpart. One launch when the GEMM plan is a single
// pass of 128-row tiles (statistics in the store epilogue); otherwise split-K slabs +
// k_bn_fwd_partial. prow: the rows of `in` through a row table (zero-copy rows).
template <typename T>
void linear_pre_bn(const Ctx<T>& c, const BnPass& p, int i, const T* in, int64_t ldin, int K, int64_t ldw,
                   const int32_t* prow = nullptr) {
  const Layout& l = c.lo;
  const int H = (int)c.d.H;
  const float* bias = p.prm + c.d.off[kBlk[i][1]];
  GemmArgs<T> g{in, ldin, c.t(l.shadow(i)), ldw, p.B, H, K, p.Bp, H, 0};
  StoreEpi bn;
  bn.mode = p.train ? 1 : 0, bn.part = (float2*)c.f(l.bnpart), bn.ldp = H;
  if (!prow && launch_gemm_bn<T>(g, c.f(l.Y[i]), H, bias, bn, c.s)) return;
  g.prow = prow;
  if (prow) g.idx_lim = c.res_rows;
  const int S = gemm_to_slabs(c, g, H);
  launch_bn_fwd_partial(c.f(c.slab_off), S, (int64_t)p.Bp * H, H, bias, p.B, H, c.f(l.Y[i]), c.f(l.bnpart), c.s);
}

// BatchNorm + ReLU of layer i: Y_i and its partials -> A_i
template <typename T>
void bn_apply(const Ctx<T>& c, const BnPass& p, int i) {
  const Layout& l = c.lo;
  const int H = (int)c.d.H;
  double* syncb = (double*)(c.ws + l.syncb);
  if (p.sync) {  // SyncBN: this rank's column sums -> all-reduce -> the global batch's statistics
    launch_bn_sync_pack(c.f(l.bnpart), p.B, H, 0, syncb, c.s);
    c.st.allreduce(syncb, 2 * H + 2, c.s);
  }
  float* run = p.bn + (int64_t)i * 2 * H;
  launch_bn_fwd_apply<T>(c.f(l.Y[i]), H, c.f(l.bnpart), p.B, p.Bp, H, p.train, p.prm + c.d.off[kBlk[i][2]],
                         p.prm + c.d.off[kBlk[i][3]], run, run + H, p.save ? c.f(l.save[i]) : nullptr, c.t(l.A[i]),
                         c.s, p.sync ? syncb : nullptr);
}

template <typename T>
void bn_layer(const Ctx<T>& c, const BnPass& p, int i, const T* in, int64_t ldin, int K, int64_t ldw) {
  linear_pre_bn<T>(c, p, i, in, ldin, K, ldw);
  bn_apply<T>(c, p, i);
}

// Encoder half. The batch's rows: in place through c.ridx, already `staged` by the previous training
// call, or gathered into the input slot (with their bit-packed target when `target_bits`). Then
// layers 0-2 and the heads GEMM + reparameterisation with b->eps: HD = mu | logvar, Z.
template <typename T>
void encoder_half(const Ctx<T>& c, const gm2_batch* b, const BnPass& p, const X3Plan& xp, bool target_bits,
                  bool staged = false, bool with_grad = false) {
  const Dims& d = c.d;
  const Layout& l = c.lo;
  const int B = p.B, Bp = p.Bp, H = (int)d.H, L = (int)d.L;
  const int64_t Gq = l.Gq;
  if (c.ridx)
    launch_resident_rows(b->rows, B, (int)round_up(d.Bm, 2 * kTile), b->resident_rows, const_cast<int32_t*>(c.ridx),
                         c.s);
  else if (!staged)
    launch_gather_rows<T>(b->data, b->ld_data, b->rows, B, (int)d.G, c.t(c.xo), d.Gp, (int)d.Gp, Bp,
                          target_bits ? (uint32_t*)(c.ws + c.xbo) : nullptr, target_bits ? d.Gp / 32 : 0, c.s);
  // bf16x3: X as (x | x) for a split input layer, and once more plain for a split dWe0 in the
  // backward (also beside the exact input layer: X in bf16 all the same)
  const bool keep_x = with_grad && xp.dwe0;
  if (xp.enc0 || keep_x)
    launch_split_kmajor(c.f(c.xo), d.Gp, B, (int)d.G, xp.Bq, (int)Gq, c.h(l.x3xd), 2 * Gq, 1,
                        keep_x ? c.h(l.x3x) : nullptr, Gq, c.s);
  if (xp.enc0) {
    // the fp32 weight shadow split per call (an Adam step or a shadow sync in between is always seen)
    launch_split_kmajor(c.f(l.sE0), d.Gp, H, (int)d.G, H, (int)Gq, c.h(l.x3w0), 2 * Gq, 0, nullptr, 0, c.s);
    const int S = gemm_to_slabs(c, xp.g_enc0, H);
    launch_bn_fwd_partial(c.f(c.slab_off), S, (int64_t)xp.Bq * H, H, p.prm + d.off[E0B], B, H, c.f(l.Y[0]),
                          c.f(l.bnpart), c.s);
  } else {
    linear_pre_bn<T>(c, p, 0, c.ridx ? c.xres : c.t(c.xo), c.ridx ? c.ld_xres : d.Gp, (int)d.Gp, d.Gp, c.ridx);
  }
  // a queued output-layer Adam update of the previous step starts here, beside the hidden layers
  // (HBM-bound next to latency-bound small GEMMs; the gather and the input-layer GEMM before this
  // point leave it nothing: one is HBM-bound too, the other holds every CU's registers)
  c.st.kick(c.s);
  bn_apply<T>(c, p, 0);
  bn_layer<T>(c, p, 1, c.t(l.A[0]), H, H, H);
  bn_layer<T>(c, p, 2, c.t(l.A[1]), H, H, H);
  const int S = gemm_to_slabs(c, GemmArgs<T>{c.t(l.A[2]), H, c.t(l.sHD), H, B, 2 * L, H, Bp, (int)d.L2r, 0}, 2 * L);
  launch_reparam<T>(c.f(l.slabs), S, (int64_t)Bp * 2 * L, L, p.prm + d.off[MUB], p.prm + d.off[LVB], b->eps, B, Bp,
                    c.f(l.HD), c.t(l.Z), d.Lr, nullptr, 0, 0, c.f(l.klpart), c.s);
}

// Decoder half: Z [Bp][Lr] through layers 3-5 -> A5
template <typename T>
void decoder_half(const Ctx<T>& c, const BnPass& p) {
  const Layout& l = c.lo;
  const int H = (int)c.d.H;
  bn_layer<T>(c, p, 3, c.t(l.Z), c.d.Lr, (int)c.d.Lp, c.d.Lr);
  bn_layer<T>(c, p, 4, c.t(l.A[3]), H, H, H);
  bn_layer<T>(c, p, 5, c.t(l.A[4]), H, H, H);
}

// mu / logvar [B][L] of the last encoder half (HD = mu | logvar) -> the caller's buffers
template <typename T>
void copy_heads(const Ctx<T>& c, int64_t B, float* mu, float* logvar) {
  const int64_t L = c.d.L;
  const float* hd = c.f(c.lo.HD);
  if (mu) HIP_OK(hipMemcpy2DAsync(mu, L * 4, hd, 2 * L * 4, L * 4, B, hipMemcpyDeviceToDevice, c.s));
  if (logvar) HIP_OK(hipMemcpy2DAsync(logvar, L * 4, hd + L, 2 * L * 4, L * 4, B, hipMemcpyDeviceToDevice, c.s));
}

// What one forward() call is for: the fused loss (scal, loss; with_grad: dL and grads too), or
// VAE.forward's probs [B][ld_probs] / per-strain (TP, FP, FN) counts of (p > thr), without a loss
struct FwdCall {
  int train = 0, with_grad = 0;
  const float* scal = nullptr;  // scalar block of the loss terms
  double* loss = nullptr;
  float *grads = nullptr, *probs = nullptr;
  int64_t ld_probs = 0;
  int* counts = nullptr;
  float thr = 0.5f;
  bool norm_hdr = false;  // record whether the backward takes the clip statistics (NormAhead)
  bool staged = false;    // the rows are in the input slot already (SlotState)
  std::function<void(hipStream_t)>* defer_tail = nullptr;  // receives the tail launch instead of running it
};

// forward (train or eval). Fills A_l, Y_l, save_l, HD, Z and runs the fused reconstruction-loss
// epilogue (dL when with_grad), or the probabilities / counts epilogue.
template <typename T>
void forward(const Ctx<T>& c, const gm2_batch* b, const float* prm, float* bn, const StepPlan<T>& plan,
             const FwdCall& f) {
  const Dims& d = c.d;
  const Layout& l = c.lo;
  const int B = (int)b->n;
  if (B <= 0 || B > d.Bm) throw Gm2Error("batch rows %d outside (0, batch_max=%lld]", B, (long long)d.Bm);
  const bool sync = f.train && c.st.opt.sync_bn;
  // (SyncBN: the batch statistics span every rank's rows, so one row here is fine)
  if (f.train && B < 2 && !sync) throw Gm2Error("Expected more than 1 value per channel when training (batch of 1)");
  check_batch_data(b, d, "batch");
  const int Bp = (int)round_up(B, kTile), H = (int)d.H;
  // 1, 2) strain rows, encoder blocks, heads + reparameterisation, decoder blocks (all NT GEMMs)
  const X3Plan& xp = plan.xp;
  const int64_t Gq = l.Gq;
  const BnPass p{prm, bn, B, Bp, f.train, sync, /*save=*/true};
  encoder_half<T>(c, b, p, xp, true, f.staged, f.with_grad != 0);
  decoder_half<T>(c, p);
  c.st.join(c.s);  // (a deferred output-layer update must be complete before the output layer)
  if (f.probs || f.counts) {  // 3') VAE.forward: p = sigmoid(logits) (model.py:89-90) and / or the
                              // per-strain (TP, FP, FN) of (p > thr) vs the strain's genes; no loss
    GemmArgs<T> g{c.t(l.A[5]), H, c.t(l.sD3), H, B, (int)d.G, H, Bp, (int)d.Gp, 0};
    MaskOut o;
    o.probs = f.probs, o.ldpr = f.ld_probs;
    o.counts = f.counts, o.xbits = (const uint32_t*)(c.ws + c.xbo), o.ldxb = d.Gp / 32;
    o.thr = f.thr;
    launch_gemm_mask<T>(g, prm + d.off[D9B], o, false, c.s);
    return;
  }
  // 3) output layer + reconstruction loss (+ dlogits), computed as logit^T: genes x strains
  GemmArgs<T> g{c.t(l.sD3), H, c.t(l.A[5]), H, (int)d.G, B, H, (int)d.Gp, Bp, 0};
  if (c.ridx) g.idx_lim = c.res_rows;
  if (xp.loss) {
    launch_split_kmajor(c.f(l.sD3), H, (int)d.G, H, (int)Gq, H, c.h(l.x3w9k), 2 * H, 0, nullptr, 0, c.s);
    launch_split_kmajor(c.f(l.A[5]), H, B, H, xp.Bq, H, c.h(l.x3a5k), 2 * H, 0, nullptr, 0, c.s);
    launch_gemm_recon_loss_x3(xp.g_loss, prm + d.off[D9B], (const uint32_t*)(c.ws + c.xbo), d.Gp / 32, f.with_grad,
                              f.scal, c.f(l.dL), d.Gp, (int)d.Gp, Bp, c.f(l.losspart), c.f(l.colpart), d.Gp, c.s);
  } else  // (zero-copy rows: the resident matrix's target bits through the row table)
    launch_gemm_recon_loss<T>(g, prm + d.off[D9B], c.ridx ? c.xbres : (const uint32_t*)(c.ws + c.xbo),
                              c.ridx ? c.ld_xbres : d.Gp / 32, f.with_grad, f.scal, c.t(l.dL), d.Gp,
                              c.f(l.losspart), c.f(l.colpart), d.Gp, c.s, c.ridx);
  // the training call: record whether its backward takes the clip statistics
  const int na_ok = f.norm_hdr && plan.norm_ahead ? 1 : 0, na_n = f.norm_hdr ? plan.bg.n9 + plan.bg.n0 : 0;
  // 4) loss slot sums + the output bias's gradient (column sums of dL): nothing in the backward
  // reads them before its final join, so a training call hands the launch to the backward, which
  // puts it on the side stream behind its first fork (off the critical path, one launch and its
  // gap fewer on the caller's stream)
  const int nlp = xp.loss ? (int)(Gq / 256) * (xp.Bq / 256) : gemm_recon_grid_blocks<T>(g);
  const int nkp = Bp / kReparamRows, rt = xp.loss ? xp.Bq / 256 : gemm_recon_row_tiles<T>(g);
  const float *lpart = c.f(l.losspart), *kpart = c.f(l.klpart), *cpart = c.f(l.colpart);
  const int64_t Gp = d.Gp, G = d.G;
  double* loss = f.loss;
  float* bgrad = f.with_grad ? f.grads + d.off[D9B] : nullptr;
  int* hdr = f.norm_hdr ? (int*)(c.ws + l.nahdr) : nullptr;
  auto tail = [=](hipStream_t s) {
    launch_fwd_tail(lpart, nlp, kpart, nkp, loss, cpart, rt, Gp, G, bgrad, hdr, na_ok, na_n, s);
  };
  if (f.defer_tail && !sched_env().tail_main) *f.defer_tail = tail;
  else tail(c.s);
}

// The next training batch's gather, staged into the other input slot (gm2_batch.next)
struct NextStage {
  const gm2_batch* b = nullptr;
  int64_t xo = 0, xbo = 0;
  hipEvent_t done = nullptr;
};

// What one backward() call adds to the plain backward of the fused loss
struct BwdCall {
  const float *dmu_ext = nullptr, *dlv_ext = nullptr;  // d(mu), d(logvar) from outside the fused loss
  int train = 1;
  const NextStage* next = nullptr;
  std::function<void(hipStream_t)>* fwd_tail = nullptr;  // the forward's deferred tail launch
};

// ---------------------------------------------------------------------------------------------
// The backward schedule, in named stages. The caller's stream runs the chain dA5 -> BatchNorm
// backward -> dX -> ... down to the input layer; weight gradients and bias sums go to a side stream:
// they are off the critical path and fill the tails of the chain's launches, and the join at the end
// orders them before the caller's work. Every operand is read in the layout its producer wrote:
// weight gradients use MN-major P and Q (dW[out][in] = sum_b dY[b][out] * in[b][in]), input gradients
// an MN-major weight (dX[b][in] = sum_out dY[b][out] * W[out][in]).
// ---------------------------------------------------------------------------------------------
// what the stages of one backward share
template <typename T>
struct BwdPass {
  const float* prm;
  float* gr;
  int B, Bp, H;
  int train;    // BatchNorm ran on batch statistics
  bool sync;    // SyncBN: the batch-coupling sums span every rank's rows
  // c: the caller's stream, whose slab area carries each dX result to the next BatchNorm backward.
  // w: the side work's context, with the split-K scratch of its own (Layout::side_slabs, side_cap) on
  // the side stream; GM2_OPT_SIDE_STREAM = 0: the same scratch and capacity on the caller's stream, so
  // side work launched while a dX result is still unread (dW9 at an even GM2_DW9_AT) leaves it alone
  // and every split count is the side stream's.
  Ctx<T> c, w;
  bool sr;  // w is a stream of its own
  // fork: the side stream waits for everything on the caller's stream so far
  void fork() const {
    if (sr) c.st.order(c.s, w.s);
  }
  // bias-gradient partials of layer i (6: the heads), each in a slice of its own: summed on the side stream
  float* col_partials(int i) const { return c.f(c.lo.colbwd) + (int64_t)i * c.lo.colbwd_cap; }
};

// what a dX GEMM leaves in the caller's stream's slab area for BatchNorm j's backward: S split-K slabs
// of `slab` elements; have_part: the GEMM's epilogue took BatchNorm j's backward partials already
struct DxOut {
  int S;
  bool have_part;
  int64_t slab;
};

// dA_j = dY . W (K-major dY, MN-major W) into the slab area, on the caller's stream; when the plan
// allows, the epilogue also takes BatchNorm j's backward partials (sum do, sum (y-mean) do). The
// mirror of linear_pre_bn.
template <typename T>
DxOut dx_pre_bn(const BwdPass<T>& p, const T* dY, int64_t lddy, const T* W, int64_t ldw, int K, int j) {
  const Ctx<T>& c = p.c;
  const Layout& l = c.lo;
  const int H = p.H;
  GemmArgs<T> g{dY, lddy, W, ldw, p.B, H, K, p.Bp, H, 0, 1, 0};
  StoreEpi bn;
  bn.mode = 2, bn.part = (float2*)c.f(l.bnpart), bn.ldp = H, bn.Y = c.f(l.Y[j]), bn.ldy = H, bn.H = H;
  bn.save = c.f(l.save[j]), bn.gamma = p.prm + c.d.off[kBlk[j][2]], bn.beta = p.prm + c.d.off[kBlk[j][3]];
  const bool part = launch_gemm_bn<T>(g, c.f(c.slab_off), H, nullptr, bn, c.s);
  return {part ? 1 : gemm_to_slabs(c, g, H), part, (int64_t)p.Bp * H};
}

// dA5[b][h] = sum_g dL[b][g] W9[g][h]; bf16x3: dL K-major and W9 MN-major (its natural [G][H] rows
// interleaved) split on the caller's stream, three products to slabs of Bq rows
template <typename T>
DxOut da5(const BwdPass<T>& p, const X3Plan& xp) {
  const Ctx<T>& c = p.c;
  const Layout& l = c.lo;
  const int H = p.H, G = (int)c.d.G, Gp = (int)c.d.Gp, Gq = (int)l.Gq;
  if (!xp.da5) return dx_pre_bn<T>(p, c.t(l.dL), Gp, c.t(l.sD3), H, Gp, 5);
  launch_split_kmajor(c.f(l.dL), Gp, p.B, G, xp.Bq, Gq, c.h(l.x3dlk), 2 * (int64_t)Gq, 0, nullptr, 0, c.s);
  launch_split_rows(c.f(l.sD3), H, G, H, Gq, H, c.h(l.x3w9m), H, c.s);
  return {gemm_to_slabs(c, xp.g_da5, H, true), false, (int64_t)xp.Bq * H};
}

// BatchNorm + ReLU backward of layer i, on the caller's stream: the partial kernel when dA_i's
// epilogue did not take the partials (it also sums split-K slabs into DA), the SyncBN pack and
// all-reduce, then the apply: dA_i -> dY_i, the BatchNorm parameter gradients, the bias partials.
// The mirror of bn_apply.
template <typename T>
void bn_bwd(const BwdPass<T>& p, int i, const DxOut& dx) {
  const Ctx<T>& c = p.c;
  const Layout& l = c.lo;
  const int H = p.H;
  const int64_t og = c.d.off[kBlk[i][2]], ob = c.d.off[kBlk[i][3]];  // gamma, beta
  float* dA = dx.S > 1 ? c.f(l.DA) : nullptr;
  if (!dx.have_part)
    launch_bn_bwd_partial(c.f(c.slab_off), dx.S, dx.slab, c.f(l.Y[i]), H, c.f(l.save[i]), p.prm + og, p.prm + ob, p.B,
                          H, c.f(l.bnpart), dA, c.s);
  double* syncb = p.sync ? (double*)(c.ws + l.syncb) : nullptr;
  if (p.sync) {  // SyncBN: the batch-coupling sums of the backward over every rank's rows
    launch_bn_sync_pack(c.f(l.bnpart), p.B, H, 1, syncb, c.s);
    c.st.allreduce(syncb, 2 * H + 2, c.s);
  }
  // (input layer, bf16: its only consumer is dWe0, which reads dY0 transposed -- written that way
  // by the same pass instead of through a transpose launch)
  T* dYT = i == 0 && sizeof(T) == 2 ? c.t(l.dYT0) : nullptr;
  launch_bn_bwd_apply<T>(dA ? dA : c.f(c.slab_off), c.f(l.Y[i]), H, c.f(l.bnpart), p.B, p.Bp, H, p.train,
                         c.f(l.save[i]), p.prm + og, p.prm + ob, p.gr + og, p.gr + ob, c.t(l.dY[i]), p.col_partials(i),
                         c.s, syncb, dYT, p.Bp);
}

// Side stream, item i of the chain. Layer i: its bias gradient (column sum of the apply's partials)
// and weight gradient dW_i = dY_i^T . in_i (layer 3: in = Z; the input layer's own is
// input_weight_grad). kHeadsItem: the head biases' column sum, then the MUW | LVW gradient from dH.
constexpr int kHeadsItem = 6;
template <typename T>
void side_layer(const BwdPass<T>& p, int i) {
  const Ctx<T>& w = p.w;
  const Layout& l = w.lo;
  const Dims& d = w.d;
  const int H = p.H, Bp = p.Bp, L = (int)d.L, Lr = (int)d.Lr, L2r = (int)d.L2r;
  float* gr = p.gr;
  if (i == kHeadsItem) {
    launch_colsum(p.col_partials(i), Bp / kReparamRows, 2 * L, 2 * L, gr + d.off[MUB], gr + d.off[LVB], L, w.s);
    gemm_to(w, GemmArgs<T>{w.t(l.dH), L2r, w.t(l.A[2]), H, 2 * L, H, Bp, L2r, H, 0, 0, 0}, gr + d.off[MUW],
            gr + d.off[LVW], L, H);
    return;
  }
  launch_colsum(p.col_partials(i), Bp / 64, H, H, gr + d.off[kBlk[i][1]], nullptr, 0, w.s);
  if (i == 0) return;
  const T* dY = w.t(l.dY[i]);
  float* dW = gr + d.off[kBlk[i][0]];
  if (i == 3) gemm_to(w, GemmArgs<T>{dY, H, w.t(l.Z), Lr, H, L, Bp, H, Lr, 0, 0, 0}, dW, nullptr, 0, L);
  else gemm_to(w, GemmArgs<T>{dY, H, w.t(l.A[i - 1]), H, H, H, Bp, H, H, 0, 0, 0}, dW, nullptr, 0, H);
}

// The fork point of side item `id` (in chain order: 5, 4, 3, the heads, 2, 1, 0): the side stream
// waits for the chain so far, then takes the items held back before and this one. `hold`
// (GM2_FORK_HOLD, SchedEnv): no fork here, the item waits for the next fork taken. Without a side
// stream nothing is held.
struct HeldItems {
  int id[7], n = 0;
};
template <typename T>
void fork_side(const BwdPass<T>& p, HeldItems& held, bool hold, int id) {
  if (hold && p.sr) {
    held.id[held.n++] = id;
    return;
  }
  p.fork();
  for (int k = 0; k < held.n; ++k) side_layer<T>(p, held.id[k]);
  held.n = 0;
  side_layer<T>(p, id);
}

// Latent bottleneck, on the caller's stream: dZ = dY3 . W_D0 to slabs, then back through the
// reparameterisation: dH = d(mu | logvar) (with the KL terms of scal and any external dmu / dlogvar)
// and the head biases' partials
template <typename T>
void latent_dx(const BwdPass<T>& p, const float* eps, const float* scal, const BwdCall& bw) {
  const Ctx<T>& c = p.c;
  const Layout& l = c.lo;
  const int H = p.H, L = (int)c.d.L, Lr = (int)c.d.Lr;
  const int S = gemm_to_slabs(c, GemmArgs<T>{c.t(l.dY[3]), H, c.t(l.sD0), Lr, p.B, L, H, p.Bp, Lr, 0, 1, 0}, L);
  launch_reparam_bwd<T>(c.f(c.slab_off), S, (int64_t)p.Bp * L, L, c.f(l.HD), eps, scal, p.B, p.Bp, L, c.t(l.dH),
                        (int)c.d.L2r, bw.dmu_ext, bw.dlv_ext, p.col_partials(kHeadsItem), c.s);
}

// Output-layer weight gradient (gradient bucket 0), on the side stream behind a fork of its own, the
// forward's deferred tail (loss slot sums, output bias gradient, norm-ahead header) right in front
// of it: dW9[g][h] = sum_b dL[b][g] A5[b][h], written as dW9^T[h][g] = sum_b A5^T[h][b] dL[b][g]
// with A5^T K-major (a transposed copy made here) and dL MN-major, stored transposed: one
// transposed-read operand instead of two (the 256x256 tile is LDS-read bound with two). Plans with
// split-K keep the both-MN-major form.
// Its place is behind the GM2_DW9_AT-th kernel of the caller's stream's chain (0 = dA5, 1 = layer 5's
// BatchNorm backward apply, 2 = the first hidden dX GEMM, ...). Alongside dA5 it would take the CUs
// dA5 needs; after it, its 860 tiles start as the hidden chain's first kernels do (the chain's head
// start is the gap the position leaves), and the tail runs on CUs dA5 no longer holds (right after
// the first fork it starved beside dA5 for ~360 us and held dW9 back,
// profiles/r04_fwd_tail_after_dw9.txt). Default 2 with dW9 on its capped grid (GM2_OPT_GRID_CAP bit 1,
// 215 workgroups x 4 tiles): the chain's BatchNorm partial and apply run before dW9 takes 215 CUs,
// and 41 CUs stay with the chain -- 6 of 6 same-box pairs faster than 0 on the full grid
// (profiles/r05_dw9_cap_ab.txt). (Last instead, beside dWe0, measured the same step time on one GPU;
// first keeps gradient bucket 0 early for the data-parallel exchange.)
template <typename T>
void output_weight_grad(const BwdPass<T>& p, const StepPlan<T>& plan, std::function<void(hipStream_t)>* fwd_tail) {
  const Ctx<T>&c = p.c, &w = p.w;
  const Layout& l = c.lo;
  const int H = p.H, G = (int)c.d.G, Gp = (int)c.d.Gp, Gq = (int)l.Gq;
  const X3Plan& xp = plan.xp;
  float* dW9 = p.gr + c.d.off[D9W];
  p.fork();
  if (fwd_tail && *fwd_tail) {
    (*fwd_tail)(w.s);
    *fwd_tail = nullptr;
  }
  if (xp.dw9) {  // bf16x3: dL and A5 as MN-major splits (k = the batch row), both made on this stream
    launch_split_rows(c.f(l.dL), Gp, p.B, G, xp.Bq, Gq, c.h(l.x3dlm), Gq, w.s);
    launch_split_rows(c.f(l.A[5]), H, p.B, H, xp.Bq, H, c.h(l.x3a5m), H, w.s);
    gemm_to(w, xp.g_dw9, dW9, nullptr, 0, H, true);
  } else if (plan_gemm<T>(plan.bg.g9).splits == 1) {
    // (A5^T here on the side stream; on the main stream before the fork measured ~35 us/step
    // slower, profiles/r02_a5t_placement_ab.txt)
    launch_transpose<T>(c.t(l.A[5]), H, p.Bp, H, c.t(l.AT5), p.Bp, w.s);
    launch_gemm_trans<T>(plan.bg.g9, dW9, H, w.s, plan.bg.direct ? (double*)(c.ws + l.nasq) : nullptr);
  } else {
    gemm_to(w, GemmArgs<T>{c.t(l.dL), Gp, c.t(l.A[5]), H, G, H, p.Bp, Gp, H, 0, 0, 0}, dW9, nullptr, 0, H);
  }
  if (c.st.opt.grad_buckets) HIP_OK(hipEventRecord(c.st.bucket[0], w.s));
}

// Quarter q of the input-layer weight gradient (gradient bucket 2 + q) is final on `s`; `rest`: so
// are the quarters after it (one launch wrote them all), which share its event
void input_quarters_final(WsState& st, hipStream_t s, int q, bool rest) {
  if (st.opt.grad_buckets) HIP_OK(hipEventRecord(st.bucket[2 + q], s));
  for (int k = q; k < (rest ? 4 : q + 1); ++k) st.bucket_ev[2 + k] = 2 + q;
}

// Input-layer weight gradient, on the caller's stream (nothing is left to overlap):
// dWe0[h][g] = sum_b dY0^T[h][b] X[b][g], dY0^T a K-major copy (bf16: bn_bwd wrote it), X MN-major.
// Gradient bucket 1 (every hidden-layer tensor) is final when the side stream's queue so far is; dWe0
// starts without waiting for it (the join follows the dWe0 launch: the side stream's last small GEMM
// and column sums run beside dWe0's first tiles instead of before them).
template <typename T>
void input_weight_grad(const BwdPass<T>& p, const StepPlan<T>& plan) {
  const Ctx<T>& c = p.c;
  const Layout& l = c.lo;
  WsState& st = c.st;
  const int H = p.H, G = (int)c.d.G;
  const X3Plan& xp = plan.xp;
  const BigGrads<T>& bg = plan.bg;
  float* dW0 = p.gr + c.d.off[E0W];
  if (sizeof(T) != 2 && !xp.dwe0) launch_transpose<T>(c.t(l.dY[0]), H, p.Bp, H, c.t(l.dYT0), p.Bp, c.s);
  if (st.opt.grad_buckets) HIP_OK(hipEventRecord(st.bucket[1], p.w.s));
  if (!xp.dwe0 && input_chunked(bg, H)) {  // four row-quarter launches, bucket 2 + q final after launch q
    for (int q = 0; q < 4; ++q) {
      GemmArgs<T> gq = bg.g0;
      const int r0 = (int)input_quarter_row(c.d, q);
      gq.P = bg.g0.P + (int64_t)r0 * bg.g0.ldp;
      gq.M = gq.Mp = H / 4;
      if (!launch_gemm_sq<T>(gq, dW0 + (int64_t)r0 * G, G, nullptr, c.s, true))
        throw Gm2Error("input-layer quarter GEMM: not a one-pass plan");
      input_quarters_final(st, c.s, q, false);
    }
    return;
  }
  if (xp.dwe0) {  // bf16x3: dY0 as an MN-major split, X's rows (exact in bf16) named twice by the row table
    launch_split_rows(c.f(l.dY[0]), H, p.B, H, xp.Bq, H, c.h(l.x3dy0), H, c.s);
    launch_dup_rows((int32_t*)(c.ws + l.x3rows), 2 * xp.Bq, c.s);
    gemm_to(c, xp.g_dwe0, dW0, nullptr, 0, G, true);
  } else if (!bg.direct || !launch_gemm_sq<T>(bg.g0, dW0, G, (double*)(c.ws + l.nasq) + bg.n9, c.s, false)) {
    gemm_to(c, bg.g0, dW0, nullptr, 0, G);
  }
  input_quarters_final(st, c.s, 0, true);  // one GEMM: buckets 2..5 become final together
}

// The next batch's rows -> the other input slot (gm2_batch.next), on the side stream behind a fork
// placed after dWe0 (beside it, the gather only slows the GEMM down by its own length; that slot's
// readers, the previous step, are earlier): under the data-parallel exchange of the input-layer
// gradient, or beside the clip / Adam passes on one GPU. Joined back before the call returns: the
// caller's stream orders every write this call makes (workspace lifetime; no device-wide sync is
// needed); the clip / Adam passes that follow wait for it, which measured time-neutral (both are
// HBM-bound) and keeps the gather beside the exchange, which waits on bucket events instead.
template <typename T>
void stage_next(const BwdPass<T>& p, const NextStage& nx) {
  const Ctx<T>& c = p.c;
  const int G = (int)c.d.G, Gp = (int)c.d.Gp, Bn = (int)nx.b->n;
  p.fork();
  launch_gather_rows<T>(nx.b->data, nx.b->ld_data, nx.b->rows, Bn, G, c.t(nx.xo), Gp, Gp, (int)round_up(Bn, kTile),
                        (uint32_t*)(c.ws + nx.xbo), Gp / 32, p.w.s);
  HIP_OK(hipEventRecord(nx.done, p.w.s));
  if (p.sr) c.st.order(p.w.s, c.s);
}

// Backward of the fused loss (or of outside output gradients, gm2_backward_outputs): the stages
// above in launch order
template <typename T>
void backward(const Ctx<T>& c, const gm2_batch* b, const float* prm, float* gr, const float* scal,
              const StepPlan<T>& plan, const BwdCall& bw) {
  const Layout& l = c.lo;
  WsState& st = c.st;
  const SchedEnv& env = sched_env();
  const hipStream_t side = st.side_stream();
  const int B = (int)b->n, H = (int)c.d.H;
  const BwdPass<T> p{prm, gr, B, (int)round_up(B, kTile), H, bw.train, bw.train && st.opt.sync_bn,
                     c, c.side(side ? side : c.s), side != nullptr};
  HeldItems held;
  const auto hold = [&](int i) { return i >= env.fork_hold; };
  // dW9 goes behind kernel env.dw9_at of the chain: mark() follows each of them (dA5, then every
  // BatchNorm apply and dX GEMM in turn)
  int chain_pos = 0;
  bool dw9_done = false;
  const auto mark = [&] {
    if (chain_pos++ != env.dw9_at) return;
    output_weight_grad<T>(p, plan, bw.fwd_tail);
    dw9_done = true;
  };
  // 1) output layer's input gradient
  DxOut dx = da5<T>(p, plan.xp);
  mark();
  // 2) layers 5, 4: BatchNorm backward, the fork (or hold) of the layer's side work, dX
  for (int i : {5, 4}) {
    bn_bwd<T>(p, i, dx);
    mark();
    fork_side<T>(p, held, hold(i), i);
    dx = dx_pre_bn<T>(p, c.t(l.dY[i]), H, c.t(l.shadow(i)), H, H, i - 1);
    mark();
  }
  // 3) latent bottleneck: layer 3, back through the reparameterisation, the heads
  bn_bwd<T>(p, 3, dx);
  mark();
  fork_side<T>(p, held, hold(3), 3);
  latent_dx<T>(p, b->eps, scal, bw);
  fork_side<T>(p, held, hold(3), kHeadsItem);
  dx = dx_pre_bn<T>(p, c.t(l.dH), c.d.L2r, c.t(l.sHD), H, (int)c.d.K2L, 2);
  mark();
  // 4) layers 2, 1
  for (int i : {2, 1}) {
    bn_bwd<T>(p, i, dx);
    mark();
    fork_side<T>(p, held, hold(i), i);
    dx = dx_pre_bn<T>(p, c.t(l.dY[i]), H, c.t(l.shadow(i)), H, H, i - 1);
    mark();
  }
  // 5) input layer: its fork is always taken, and whatever was held goes with it
  bn_bwd<T>(p, 0, dx);
  mark();
  fork_side<T>(p, held, false, 0);
  if (!dw9_done) output_weight_grad<T>(p, plan, bw.fwd_tail);  // (GM2_DW9_AT past the chain's end: beside dWe0)
  input_weight_grad<T>(p, plan);
  // 6) join: the caller's stream sees every weight gradient
  if (p.sr) st.order(p.w.s, c.s);
  // 7) the next batch's gather
  if (bw.next) stage_next<T>(p, *bw.next);
  st.recorded = st.opt.grad_buckets != 0;
}

// The sampling decode's output layer, gated per tile (extras.py:196-201, decode + threshold).
//  * bf16x3 split: activations and output weights split into bf16 (hi | lo) per 32 columns
//    (launch_split3), and the main loop (mainloop_pp, S3) sums hi.hi + hi.lo + lo.hi -- each fp32
//    product a.w up to 3.02 x 2^-16 |a| |w| (the dropped lo.lo term and the two splits' residuals),
//    i.e. per logit at most e = 4.62e-5 ||a_r||_2 ||w_g||_2 (Cauchy-Schwarz) on top of the fp32
//    accumulation the exact path has as well.
//  * Per 256 x 256 tile (genome rows x genes) the gate takes the split form when 4.62e-5 x the
//    block's largest ||a_r|| x the block's largest ||w_g|| is at most kSplitBound (1e-3); every
//    other tile runs the exact-fp32 kernel. One large activation row or weight row thus sends only
//    its own tiles to fp32. Both kernels are launched over their full grids behind the split kernels
//    and each tile's workgroup runs only on its verdict (the rest exit at once): no call waits on the
//    host. (A host read of the maxima stalled every chunk behind the previous chunk's mask copy and
//    drained the queue: 3.0 M genomes/s end to end. The first device form gated whole chunks on the
//    global maxima, so one large row or weight sent every tile to fp32.)
//  * Certified band (SURVEY.md 7 "Hard parts" (ii)): both epilogues list the elements whose logit
//    lies within coef * ||a_r|| ||w_g|| of the threshold (MaskBand) -- where the reference's own fp32
//    arithmetic, or the split, could land on either side -- and k_band_fix recomputes each listed
//    logit in fp64 from the same fp32 activations and weights and sets its mask bit from that. The
//    counts (tiles per path, band elements, bits the recompute flipped, list overflow) accumulate in
//    the workspace (DecodeCtl) for gm2_workspace_stat.
// False: not taken (the caller runs the exact path alone, without band recompute).
bool decode_split3(const Ctx<float>& c, const float* prm, int n, uint8_t* mask, int64_t ldm, uint8_t* bits,
                   int64_t ldb) {
  const Dims& d = c.d;
  const Layout& l = c.lo;
  const int H = (int)d.H, G = (int)d.G;
  const int Bq = (int)round_up(n, 2 * kTile), Gq = (int)round_up(G, 2 * kTile);
  // Preconditions of the split kernels and the two gated output-layer kernels, checked before
  // anything is launched; when one fails the caller runs the exact path alone. The output weights
  // start at off[D9W] floats into the parameter buffer, which is 2L mod 128 floats: an odd latent
  // width leaves them only 4-B aligned (launch_split3 reads 16-B pieces). The exact kernel's packed
  // stores need ldb * 8 >= its padded gene extent, the split kernel's the 256-padded one up to ldb.
  if (!l.s3a || H % 32) return false;
  if ((((uintptr_t)(prm + d.off[D9W])) | ((uintptr_t)c.f(l.A[5]))) & 15) return false;
  if (bits && ((ldb & 15) || (((uintptr_t)bits) & 15) || ldb * 8 < d.Gp)) return false;
  if (mask && ldm < G) return false;
  // u8 masks: the decode writes packed bits only (into the workspace when the caller wants none) and
  // k_expand_bits writes the caller's rows from them in one streaming pass (the tile epilogue's own
  // u8 rows, at odd G never 16-B aligned, cost 3.4 ms more per 65,536-genome chunk,
  // profiles/r06_decode_u8_ab.txt)
  if (mask && !bits) {
    if (!l.s3bits || l.s3ldb * 8 < d.Gp) return false;
    bits = (uint8_t*)(c.ws + l.s3bits);
    ldb = l.s3ldb;
  }
  const DecodeCounters k = decode_counters(c.ws, l, Bq, Gq);
  bf16_t* a3 = (bf16_t*)(c.ws + l.s3a);
  bf16_t* w3 = (bf16_t*)(c.ws + l.s3w);
  float* rn = c.f(l.s3rn);
  float* cn = c.f(l.s3cn);
  const float* w9 = prm + d.off[D9W];
  HIP_OK(hipMemsetAsync(k.ctl_zero, 0, k.ctl_zero_bytes, c.s));
  const bool single = opts().sample_single != 0 && H % 64 == 0;  // (the single GEMM's K = H: 64-wide K-tiles)
  bf16_t* a1 = (bf16_t*)(c.ws + l.s3a1);
  bf16_t* w1 = (bf16_t*)(c.ws + l.s3w1);
  launch_split3(c.f(l.A[5]), H, n, Bq, H, a3, 2 * H, rn, k.ablk, c.s, single ? a1 : nullptr);
  launch_split3(w9, H, G, Gq, H, w3, 2 * H, cn, k.wblk, c.s, single ? w1 : nullptr);
  c.st.decode_cum = k.cum;
  c.st.decode_ovf = k.ovf_cum;
  // The three tiers' bands from one base. Entries past a shard's capacity flag their 256 x 256 block,
  // which k_band_tile_fix then recomputes whole in fp64 (no bit is left as a bf16 tier decided it).
  const int tiles = (Bq / 256) * (Gq / 256);
  MaskBand base;
  base.rn = rn, base.cn = cn;
  base.counts = k.shard_counts, base.list = (uint2*)(c.ws + l.s3band);
  base.cap = (unsigned)std::min<int>(opts().band_cap, (int)kBandShardCap);
  base.oflag = k.ovf_flags, base.olist = k.ovf_list, base.ocount = k.ovf_count;
  base.obn = Gq / 256, base.oblocks = (unsigned)tiles;
  // band half-widths per unit ||a_r|| ||w_g|| (MaskBand): single tiles carry the operands' bf16
  // rounding and the fp32 accumulation of their H products, split tiles the split's own error and the
  // fp32 accumulation of its 3H products, exact tiles the fp32 accumulation of H products; all, the
  // reference's own fp32 accumulation of H products
  const double gH = band_gamma((double)H), g3H = band_gamma(3.0 * H);
  // (the split and single kernels' tiles keep their band elements in their own slots -- the tile
  // grid is the same and each tile runs in one of them; the exact kernel's, rare, go to the shards)
  MaskBand be = base;
  be.coef = (float)(2.0 * gH);
  MaskBand bs = base;
  bs.coef = (float)(kSplitUnit * 1.01 + g3H + gH);
  bs.tlist = (uint2*)(c.ws + l.s3tlist), bs.tcount = (unsigned*)(c.ws + l.s3tcount);
  bs.tfound = k.tile_found, bs.tslots = kBandTileSlots;
  MaskBand b1 = bs;
  b1.coef = (float)(kSingleUnit * 1.01 + 2.0 * gH), b1.drop_overflow = 1, b1.tiles_done = k.tiles_single;
  HIP_OK(hipMemsetAsync(bs.tcount, 0, (size_t)tiles * 4, c.s));
  HIP_OK(hipMemsetAsync(k.ovf_zero, 0, k.ovf_zero_bytes, c.s));
  // every tier writes the packed bits alone, behind the same gate: only its verdict and counter differ
  MaskGate gate;
  gate.ablk = k.ablk, gate.wblk = k.wblk;
  gate.single = single ? 1 : 0;
  gate.single_bound = opts().single_bound_milli * 1e-3;  // (GM2_OPT_SAMPLE_SINGLE_BOUND, for A/Bs and tests)
  auto tier = [&](int run, unsigned* ran, const MaskBand& band) {
    MaskOut o;
    o.bits = bits, o.ldb = ldb;
    o.gate = gate, o.gate.run = run, o.gate.tiles = ran;
    o.band = band;
    return o;
  };
  const MaskOut split = tier(1, k.tiles_split, bs), exact = tier(2, k.tiles_exact, be);
  GemmArgs<bf16_t> g{a3, 2 * H, w3, 2 * H, n, G, 2 * H, Bq, Gq, 0};
  if (single) {  // both bf16 tiers in one launch (a single tile whose band overflows re-runs as split)
    GemmArgs<bf16_t> g1{a1, H, w1, H, n, G, H, Bq, Gq, 0};
    launch_gemm_mask_tiered(g1, g, prm + d.off[D9B], tier(3, k.tiles_single, b1), split, c.s);
  } else {
    launch_gemm_mask<bf16_t>(g, prm + d.off[D9B], split, true, c.s);
  }
  GemmArgs<float> ge{c.f(l.A[5]), H, c.f(l.sD3), H, n, G, H, (int)round_up(n, kTile), (int)d.Gp, 0};
  launch_gemm_mask<float>(ge, prm + d.off[D9B], exact, false, c.s);
  launch_band_fix(bs, tiles, c.f(l.A[5]), H, w9, H, prm + d.off[D9B], H, bits, ldb, k.flips, c.s);
  launch_band_tile_fix(bs, c.f(l.A[5]), H, w9, H, prm + d.off[D9B], H, n, G, bits, ldb, k.flips, c.s);
  launch_decode_stats(k, bs.cap, c.s);
  if (mask) launch_expand_bits(bits, ldb, n, G, mask, ldm, c.s);
  return true;
}

// Z [n][Lr] (in the workspace) -> the decoder half -> the output layer's masks / probabilities as `o`
// names them (u8 masks [n][ldm] or packed bits [n][ldb], and / or probabilities; threshold 0.5)
template <typename T>
void decode_chain(const Ctx<T>& c, const float* prm, float* bn, int n, const MaskOut& o) {
  const Dims& d = c.d;
  const Layout& l = c.lo;
  const int Bp = (int)round_up(n, kTile), H = (int)d.H;
  decoder_half<T>(c, BnPass{prm, bn, n, Bp});
  if constexpr (std::is_same_v<T, float>) {
    if (!o.probs && opts().sample_split && decode_split3(c, prm, n, o.mask, o.ldm, o.bits, o.ldb)) return;
  }
  c.st.exact_decodes++;
  GemmArgs<T> g{c.t(l.A[5]), H, c.t(l.sD3), H, n, (int)d.G, H, Bp, (int)d.Gp, 0};
  launch_gemm_mask<T>(g, prm + d.off[D9B], o, false, c.s);
}

// make `s` wait for a pending stage on `ws` and forget it (the caller is about to write slot 0)
void drop_stage(WsState& st, hipStream_t s) {
  if (st.slot.staged) HIP_OK(hipStreamWaitEvent(s, st.slot_done, 0));
  st.slot.staged = false;
}

// SyncBN, a rank with no rows in this global batch: zero gradient and loss sums, the 12 all-reduces
// with zero contributions in the order the ranks with rows issue them, and the same running-statistics
// update (the global batch's); bucket events recorded so a gradient exchange can follow
void sync_bn_no_rows(const Layout& lo, float* gr, float* bn, double* loss, void* ws, hipStream_t s, WsState& st) {
  const Dims& d = lo.d;
  const int64_t H = d.H, n = 2 * H + 2;
  double* syncb = (double*)((char*)ws + lo.syncb);
  HIP_OK(hipMemsetAsync(gr, 0, (size_t)d.off[NP] * 4, s));
  HIP_OK(hipMemsetAsync(loss, 0, 3 * sizeof(double), s));
  for (int i = 0; i < 6; ++i) {
    HIP_OK(hipMemsetAsync(syncb, 0, (size_t)n * 8, s));
    st.allreduce(syncb, n, s);
    launch_bn_sync_running(syncb, (int)H, bn + (int64_t)i * 2 * H, bn + (int64_t)i * 2 * H + H, s);
  }
  for (int i = 5; i >= 0; --i) {
    HIP_OK(hipMemsetAsync(syncb, 0, (size_t)n * 8, s));
    st.allreduce(syncb, n, s);
  }
  if (st.opt.grad_buckets)
    for (int b = 0; b < GM2_GRAD_BUCKETS; ++b) {
      HIP_OK(hipEventRecord(st.bucket[b], s));
      st.bucket_ev[b] = b;
    }
  st.recorded = st.opt.grad_buckets != 0;
}

// gm2_batch.resident usable in place for this training call: its precision, padding and alignment,
// and GEMM plans that take zero-copy rows (bf16 256x256 ping-pong); otherwise the rows are gathered
template <typename T>
bool zero_copy_ok(const Ctx<T>& c, const gm2_batch* b) {
  const Dims& d = c.d;
  if (!b->resident || b->resident_prec != c.lo.prec || sizeof(T) != 2) return false;
  if (!b->resident_bits || b->resident_rows < 0 || b->resident_rows > INT32_MAX - 1) return false;
  if (b->ld_resident < d.Gp || b->ld_resident % 64 || ((uintptr_t)b->resident & 15)) return false;
  if (b->ld_resident_bits < d.Gp / 32 || b->ld_resident_bits % 4 || ((uintptr_t)b->resident_bits & 15)) return false;
  const int B = (int)b->n, Bp = (int)round_up(B, kTile), H = (int)d.H;
  if (B < 1 || Bp % (2 * kTile)) return false;
  GemmArgs<T> enc{(const T*)b->resident, b->ld_resident, c.t(c.lo.sE0), d.Gp, B, H, (int)d.Gp, Bp, H, 0};
  enc.prow = (const int32_t*)1;
  GemmArgs<T> dwe0{c.t(c.lo.dYT0), Bp, (const T*)b->resident, b->ld_resident, H, (int)d.G, Bp, H, (int)d.Gp, 0, 1, 0};
  dwe0.qrow = (const int32_t*)1;
  return gemm_idx_ok<T>(enc) && gemm_idx_ok<T>(dwe0);
}

template <typename T>
void run_train(const Layout& lo, const gm2_batch* b, const float* prm, float* gr, float* bn, const float* scal,
               double* loss, void* ws, void* strm, WsState& st) {
  if (b->n == 0 && st.opt.sync_bn) {
    st.join((hipStream_t)strm);  // (it zeroes the whole gradient buffer)
    drop_stage(st, (hipStream_t)strm);
    sync_bn_no_rows(lo, gr, bn, loss, ws, (hipStream_t)strm, st);
    return;
  }
  Ctx<T> c(lo, ws, strm, st);
  c.x3 = lo.x3 && st.opt.train_split != 0;
  SlotState& ss = st.slot;
  bool hit = false;
  int slot = 0;
  NextStage nx;
  const gm2_batch* nb = nullptr;
  if (zero_copy_ok<T>(c, b)) {  // the resident matrix's rows in place: no gather, no staging
    c.ridx = (const int32_t*)((char*)ws + lo.ridx);
    c.xres = (const T*)b->resident, c.ld_xres = b->ld_resident;
    c.xbres = b->resident_bits, c.ld_xbres = b->ld_resident_bits;
    c.res_rows = b->resident_rows + 1;
    drop_stage(st, c.s);
  } else {
    hit = ss.staged && ss.prec == lo.prec && ss.total == lo.total && ss.data == b->data && ss.ld == b->ld_data &&
          ss.rows == b->rows && ss.n == b->n;
    slot = hit ? ss.slot : 0;
    drop_stage(st, c.s);
    c.xo = slot ? lo.X1 : lo.X;
    c.xbo = slot ? lo.XB1 : lo.XB;
    nb = b->next;
  }
  if (nb) {
    if (nb->n <= 0 || nb->n > lo.d.Bm) throw Gm2Error("next batch: rows %lld outside (0, batch_max]", (long long)nb->n);
    check_batch_data(nb, lo.d, "next batch");
    nx.b = nb, nx.done = st.slot_done;
    nx.xo = slot ? lo.X : lo.X1, nx.xbo = slot ? lo.XB : lo.XB1;
  }
  const StepPlan<T> plan = step_plan<T>(c, (int)b->n);
  if (lo.x3) {  // GM2_TSTAT_*: this call's five G-wide GEMMs
    const int n = plan.xp.count();
    st.x3_split += n;
    st.x3_exact += 5 - n;
  }
  std::function<void(hipStream_t)> tail;
  FwdCall fw;
  fw.train = fw.with_grad = 1, fw.scal = scal, fw.loss = loss, fw.grads = gr;
  fw.norm_hdr = true, fw.staged = hit, fw.defer_tail = &tail;
  forward<T>(c, b, prm, bn, plan, fw);
  BwdCall bw;
  bw.next = nb ? &nx : nullptr, bw.fwd_tail = &tail;
  backward<T>(c, b, prm, gr, scal, plan, bw);
  if (nb) {
    ss.staged = true, ss.slot = slot ^ 1;
    ss.data = nb->data, ss.ld = nb->ld_data, ss.rows = nb->rows, ss.n = nb->n;
    ss.prec = lo.prec, ss.total = lo.total;
  }
}

// guarded body of a C-ABI call on workspace `ws`: its state, with its options in scope
template <typename F>
int with_ws(void* ws, F&& f) {
  return guarded([&] {
    WsState& st = ws_state(ws);
    OptionScope scope(st.opt);
    f(st);
  });
}

// the same for a call that reads or writes parameters, moments or GEMM shadows from its first
// launch on: it first joins a deferred output-layer Adam update (the training call instead waits
// right before the output layer, so the update overlaps its first half)
template <typename F>
int with_ws_joined(void* ws, void* stream, F&& f) {
  return with_ws(ws, [&](WsState& st) {
    st.join((hipStream_t)stream);
    f(st);
  });
}

// The body of gm2_decode_mask and gm2_decode_bits (`packed`): z [n][L] through the decoder of an
// f32 workspace
int decode_rows(const gm2_dims* d, const float* params, const float* bn_running, const float* z, int64_t n,
                const MaskOut& o, bool packed, void* ws, void* stream) {
  return with_ws_joined(ws, stream, [&](WsState& st) {
    const Layout lo = make_layout(d, GM2_F32);
    if (n <= 0 || n > lo.d.Bm) throw Gm2Error("decode rows %lld outside (0, batch_max]", (long long)n);
    const bool ld_short = packed ? o.ldb < gm2_packed_row_bytes(lo.d.G) : o.ldm < lo.d.G;
    if (ld_short || (o.probs && o.ldpr < lo.d.G))
      throw Gm2Error(packed ? "decode_bits: ld too small" : "decode: ld < G");
    Ctx<float> c(lo, ws, stream, st);
    // z [n][L] -> Z [Bm][Lp] (pad columns stay zero from workspace init)
    HIP_OK(hipMemcpy2DAsync(c.f(lo.Z), lo.d.Lr * 4, z, lo.d.L * 4, lo.d.L * 4, n, hipMemcpyDeviceToDevice, c.s));
    decode_chain<float>(c, params, const_cast<float*>(bn_running), (int)n, o);
  });
}

}  // namespace

// =================================================================================================
extern "C" {

const char* gm2_last_error(void) { return g_err.c_str(); }
int gm2_abi_version(void) { return GM2_ABI_VERSION; }

int gm2_param_count(const gm2_dims* d, int64_t* n) {
  return guarded([&] { *n = make_dims(d).off[NP]; });
}

int gm2_param_offsets(const gm2_dims* d, int64_t* off) {
  return guarded([&] {
    const Dims x = make_dims(d);
    for (int i = 0; i <= NP; ++i) off[i] = x.off[i];
  });
}

int gm2_workspace_size(const gm2_dims* d, int prec, size_t* bytes) {
  return guarded([&] { *bytes = (size_t)make_layout(d, prec).total; });
}

int gm2_workspace_init(const gm2_dims* d, int prec, void* ws, size_t ws_bytes, void* stream) {
  return guarded([&] {
    const Layout lo = make_layout(d, prec);
    if ((size_t)lo.total > ws_bytes) throw Gm2Error("workspace too small: %zu < %lld", ws_bytes, (long long)lo.total);
    if ((uintptr_t)ws & 255) throw Gm2Error("workspace must be 256-B aligned");
    ws_reset(ws);  // a new (or reused) workspace: process-default options, no staged batch
    HIP_OK(hipMemsetAsync(ws, 0, (size_t)lo.total, (hipStream_t)stream));
  });
}

int gm2_sync_shadows(const gm2_dims* d, int prec, const float* params, void* ws, void* stream) {
  return with_ws_joined(ws, stream, [&](WsState& st) {
    const Layout lo = make_layout(d, prec);
    by_precision(lo.prec, [&](auto tag) {
      using T = decltype(tag);
      Ctx<T> c(lo, ws, stream, st);
      launch_shadow_sync<T>(make_table(c), params, c.s);
    });
  });
}

int gm2_resident_layout(int64_t S, int64_t G, int prec, int64_t* ld, int64_t* ld_bits, int64_t* rows_alloc,
                        size_t* bytes, size_t* bits_bytes) {
  return guarded([&] {
    if (S < 0 || S > INT32_MAX - 64 || G <= 0 || (prec != GM2_F32 && prec != GM2_BF16))
      throw Gm2Error("resident layout: S=%lld G=%lld prec=%d", (long long)S, (long long)G, prec);
    const int64_t l = round_up(G, 2 * kTile), r = round_up(S + 1, 64);
    *ld = l, *ld_bits = l / 32, *rows_alloc = r;
    *bytes = (size_t)(r * l * (prec == GM2_F32 ? 4 : 2));
    *bits_bytes = (size_t)(r * (l / 32) * 4);
  });
}

int gm2_resident_build(const uint8_t* data, int64_t ld_data, int64_t S, int64_t G, int prec, void* out,
                       uint32_t* bits, void* stream) {
  return guarded([&] {
    int64_t l = 0, lb = 0, r = 0;
    size_t by = 0, bb = 0;
    if (gm2_resident_layout(S, G, prec, &l, &lb, &r, &by, &bb) != 0) throw Gm2Error("%s", g_err.c_str());
    if (!out || !bits || ((uintptr_t)out & 15) || ((uintptr_t)bits & 15)) throw Gm2Error("resident: null or misaligned output");
    if (S > 0 && (!data || ld_data % 16 || ld_data < G || ((uintptr_t)data & 15)))
      throw Gm2Error("resident: data rows must be 16-B aligned with ld_data (%lld) a multiple of 16 and >= G",
                     (long long)ld_data);
    // the gather with identity rows: rows < S copied (0/1 -> T, target bits), rows S.. r-1 and
    // columns G.. ld-1 zero
    const uint8_t* src = S > 0 ? data : (const uint8_t*)out;
    const int64_t lds = S > 0 ? ld_data : 16;
    by_precision(prec, [&](auto tag) {
      using T = decltype(tag);
      launch_gather_rows<T>(src, lds, nullptr, (int)S, (int)G, (T*)out, l, (int)l, (int)r, bits, lb,
                            (hipStream_t)stream);
    });
  });
}

int gm2_train_fwd_bwd(const gm2_dims* d, int prec, const gm2_batch* batch, const float* params, float* grads,
                      float* bn_running, const float* scalars, double* loss, void* ws, void* stream) {
  return with_ws(ws, [&](WsState& st) {
    const Layout lo = make_layout(d, prec);
    by_precision(lo.prec, [&](auto tag) {
      run_train<decltype(tag)>(lo, batch, params, grads, bn_running, scalars, loss, ws, stream, st);
    });
  });
}

int gm2_grad_norm(const gm2_dims* d, int prec, const float* params, const float* grads, const float* scalars,
                  double* loss, void* ws, void* stream) {
  return with_ws_joined(ws, stream, [&](WsState& st) {
    const Layout lo = make_layout(d, prec);
    const int64_t n = lo.d.off[NP];
    const int nb = grad_stats_blocks(n);
    double* part = (double*)((char*)ws + lo.gradpart);
    float* clip = (float*)((char*)ws + lo.clip);
    NormAhead na;
    na.hdr = (const int*)((char*)ws + lo.nahdr), na.sq = (const double*)((char*)ws + lo.nasq);
    na.lo0 = lo.d.off[E0W], na.hi0 = lo.d.off[E0B], na.lo9 = lo.d.off[D9W], na.hi9 = lo.d.off[D9B];
    launch_grad_stats(params, grads, n, scalars, part, nb, na, (hipStream_t)stream);
    launch_grad_finalize(part, nb, scalars, clip, loss + 3, na, (hipStream_t)stream);  // loss[3], loss[4]
  });
}

int gm2_adam_step(const gm2_dims* d, int prec, float* params, const float* grads, float* m, float* v,
                  const float* scalars, void* ws, void* stream) {
  return with_ws_joined(ws, stream, [&](WsState& st) {
    const Layout lo = make_layout(d, prec);
    const float* clip = (const float*)((char*)ws + lo.clip);
    by_precision(lo.prec, [&](auto tag) {
      using T = decltype(tag);
      Ctx<T> c(lo, ws, stream, st);
      const TensorTable all = make_table(c, 1);
      if (!st.opt.defer_adam || !st.opt.side_stream) {
        launch_adam_fused<T>(all, grads, params, m, v, scalars, clip, c.s);
        return;
      }
      // every tensor but the output layer now; decoder.9.{weight,bias} (the table's last two
      // entries, half the bytes at v0) queued with a copy of the scalar block (see WsState::kick)
      float* qs = (float*)((char*)ws + lo.adamscal);
      launch_adam_fused<T>(table_range(all, 0, all.n - 2), grads, params, m, v, scalars, clip, c.s, 0, qs);
      WsState::QueuedAdam& q = st.qadam;
      q.queued = true, q.prec = lo.prec;
      q.tt = table_range(all, all.n - 2, all.n);
      q.g = grads, q.p = params, q.m = m, q.v = v, q.scal = qs, q.clip = clip;
    });
  });
}

int gm2_eval_forward(const gm2_dims* d, int prec, const gm2_batch* batch, const float* params,
                     const float* bn_running, const float* scalars, double* loss, void* ws, void* stream) {
  return with_ws_joined(ws, stream, [&](WsState& st) {
    const Layout lo = make_layout(d, prec);
    drop_stage(st, (hipStream_t)stream);  // these write input slot 0
    float* bn = const_cast<float*>(bn_running);  // eval mode never writes running stats
    by_precision(lo.prec, [&](auto tag) {
      using T = decltype(tag);
      Ctx<T> c(lo, ws, stream, st);
      c.x3 = lo.x3 && st.opt.train_split != 0;  // (x3_plan: f32 elements only)
      const StepPlan<T> plan = step_plan<T>(c, (int)batch->n);
      if (lo.x3) {  // GM2_TSTAT_*: the input layer and the output layer + loss
        const X3Plan& xp = plan.xp;
        st.x3_split += (int)xp.enc0 + (int)xp.loss;
        st.x3_exact += 2 - ((int)xp.enc0 + (int)xp.loss);
      }
      FwdCall fw;
      fw.scal = scalars, fw.loss = loss;
      forward<T>(c, batch, params, bn, plan, fw);
    });
  });
}

int gm2_decode_mask(const gm2_dims* d, const float* params, const float* bn_running, const float* z, int64_t n,
                    uint8_t* mask, int64_t ld_mask, float* probs, int64_t ld_probs, void* ws, void* stream) {
  MaskOut o;
  o.mask = mask, o.ldm = ld_mask, o.probs = probs, o.ldpr = ld_probs;
  return decode_rows(d, params, bn_running, z, n, o, false, ws, stream);
}

int64_t gm2_packed_row_bytes(int64_t G) { return round_up(G, kTile) / 8; }

int gm2_mask_count_groups(const uint8_t* bits, int64_t n, int64_t ld_bits, const int32_t* group_offsets,
                          int64_t n_groups, const int32_t* positions, int32_t* counts, void* stream) {
  return guarded([&] {
    if (n < 0 || n_groups < 0 || (n && (!bits || !counts)) || (n_groups && (!group_offsets || !positions)))
      throw Gm2Error("mask_count_groups: bad arguments");
    if (n_groups == 0) {
      HIP_OK(hipMemsetAsync(counts, 0, (size_t)n * 4, (hipStream_t)stream));
      return;
    }
    launch_count_groups(bits, n, ld_bits, group_offsets, n_groups, positions, counts, (hipStream_t)stream);
  });
}

int gm2_mask_row_offsets(const uint8_t* bits, int64_t n, int64_t ld_bits, const uint8_t* keep_bits, int64_t* offsets,
                         void* stream) {
  return guarded([&] {
    if (n < 0 || !offsets || (n && !bits) || (ld_bits & 15)) throw Gm2Error("mask_row_offsets: bad arguments");
    launch_row_offsets(bits, n, ld_bits, keep_bits, offsets, (hipStream_t)stream);
  });
}

int gm2_mask_compact(const uint8_t* bits, int64_t n, int64_t ld_bits, const uint8_t* keep_bits, const int64_t* offsets,
                     int32_t* indices, void* stream) {
  return guarded([&] {
    if (n < 0 || (n && (!bits || !offsets)) || (ld_bits & 15)) throw Gm2Error("mask_compact: bad arguments");
    launch_compact(bits, n, ld_bits, keep_bits, offsets, indices, (hipStream_t)stream);
  });
}

namespace {
// the gene count of packed rows: the kernels index bits with 32-bit integers
void check_gene_count(const char* what, int64_t G) {
  if (G < 1 || G > 0x7fffffff) throw Gm2Error("%s: G %lld outside [1, 2^31)", what, (long long)G);
}
// one operand of the bit-row cross products: n rows of pitch ld, 16-B aligned, covering G bits
void check_bit_rows(const char* what, const char* name, const uint8_t* p, int64_t n, int64_t ld, int64_t G) {
  if (n < 0) throw Gm2Error("%s: negative row count of %s (%lld)", what, name, (long long)n);
  if (ld <= 0 || (ld & 15) || ld * 8 < G)
    throw Gm2Error("%s: pitch of %s (%lld) must be a multiple of 16 bytes covering G = %lld bits", what, name,
                   (long long)ld, (long long)G);
  if ((uintptr_t)p & 15) throw Gm2Error("%s: rows of %s must be 16-B aligned", what, name);
  if (n && !p) throw Gm2Error("%s: null %s", what, name);
}
}  // namespace

int gm2_mask_cooccur(const uint8_t* a, int64_t na, int64_t lda, const uint8_t* b, int64_t nb, int64_t ldb, int64_t G,
                     int32_t* out, int64_t ldo, void* stream) {
  return guarded([&] {
    check_gene_count("mask_cooccur", G);
    check_bit_rows("mask_cooccur", "a", a, na, lda, G);
    check_bit_rows("mask_cooccur", "b", b, nb, ldb, G);
    if (ldo < nb) throw Gm2Error("mask_cooccur: ldo %lld < nb %lld", (long long)ldo, (long long)nb);
    if ((uintptr_t)out & 3) throw Gm2Error("mask_cooccur: out must be 4-B aligned");
    if (na == 0 || nb == 0) return;
    if (!out) throw Gm2Error("mask_cooccur: null out");
    launch_bit_cooccur(a, na, lda, b, nb, ldb, G, out, ldo, (hipStream_t)stream);
  });
}

int gm2_mask_nearest(const uint8_t* q, int64_t nq, int64_t ldq, const uint8_t* ref, int64_t nr, int64_t ldr, int64_t G,
                     int64_t* best, void* stream) {
  return guarded([&] {
    check_gene_count("mask_nearest", G);
    check_bit_rows("mask_nearest", "q", q, nq, ldq, G);
    check_bit_rows("mask_nearest", "ref", ref, nr, ldr, G);
    if (nr == 0) throw Gm2Error("mask_nearest: no reference rows (nr = 0)");
    if (nr > 0x7fffffff) throw Gm2Error("mask_nearest: nr %lld does not fit the 32-bit index", (long long)nr);
    if ((uintptr_t)best & 7) throw Gm2Error("mask_nearest: best must be 8-B aligned");
    if (nq == 0) return;
    if (!best) throw Gm2Error("mask_nearest: null best");
    launch_bit_nearest(q, nq, ldq, ref, nr, ldr, G, best, (hipStream_t)stream);
  });
}

int gm2_mask_gene_counts(const uint8_t* bits, int64_t n_rows, int64_t ld_bits, int64_t G, const int32_t* rows, int64_t n,
                         int64_t* counts, int accumulate, void* stream) {
  return guarded([&] {
    check_gene_count("mask_gene_counts", G);
    if (n < 0) throw Gm2Error("mask_gene_counts: negative n (%lld)", (long long)n);
    check_bit_rows("mask_gene_counts", "bits", bits, n_rows, ld_bits, G);
    if (!rows && n > n_rows)
      throw Gm2Error("mask_gene_counts: n %lld > n_rows %lld without an index list", (long long)n, (long long)n_rows);
    if (rows && n && n_rows == 0) throw Gm2Error("mask_gene_counts: an index list into n_rows = 0 rows");
    if ((uintptr_t)rows & 3) throw Gm2Error("mask_gene_counts: rows must be 4-B aligned");
    if ((uintptr_t)counts & 7) throw Gm2Error("mask_gene_counts: counts must be 8-B aligned");
    if (!counts) throw Gm2Error("mask_gene_counts: null counts");
    if (n == 0 && accumulate) return;
    if (!accumulate) HIP_OK(hipMemsetAsync(counts, 0, (size_t)G * 8, (hipStream_t)stream));
    launch_gene_counts(bits, n_rows, ld_bits, G, rows, n, counts, (hipStream_t)stream);
  });
}

int gm2_mask_transpose(const uint8_t* bits, int64_t n, int64_t ld_bits, int64_t G, uint8_t* out, int64_t ld_out,
                       void* stream) {
  return guarded([&] {
    check_gene_count("mask_transpose", G);
    if (n > 0x7fffffff) throw Gm2Error("mask_transpose: n %lld outside [0, 2^31)", (long long)n);
    check_bit_rows("mask_transpose", "bits", bits, n, ld_bits, G);
    if (ld_out <= 0 || (ld_out & 15) || ld_out < (n + 7) / 8)
      throw Gm2Error("mask_transpose: pitch of out (%lld) must be a multiple of 16 bytes covering n = %lld bits",
                     (long long)ld_out, (long long)n);
    if ((uintptr_t)out & 15) throw Gm2Error("mask_transpose: rows of out must be 16-B aligned");
    if (n == 0) return;
    if (!out) throw Gm2Error("mask_transpose: null out");
    // the bytes read: rows of roundup(G, 128) / 8; the bytes written: G rows of roundup(n, 128) / 8
    const uintptr_t b0 = (uintptr_t)bits, b1 = b0 + (uintptr_t)((n - 1) * ld_bits + gm2_packed_row_bytes(G));
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((G - 1) * ld_out + gm2_packed_row_bytes(n));
    if (b0 < o1 && o0 < b1) throw Gm2Error("mask_transpose: out and bits overlap");
    launch_bit_transpose(bits, n, ld_bits, G, out, ld_out, (hipStream_t)stream);
  });
}

int gm2_mask_minimized_stats(const uint8_t* bits, int64_t n, int64_t ld_bits, int64_t G, const int32_t* feat_col,
                             const int32_t* feat_start, const int32_t* feat_end, int64_t F, int64_t* removed_bp,
                             int32_t* genes_removed, uint64_t* signature, void* stream) {
  return guarded([&] {
    check_gene_count("mask_minimized_stats", G);
    if (F < 0 || F > 0x7fffffff) throw Gm2Error("mask_minimized_stats: F %lld outside [0, 2^31)", (long long)F);
    check_bit_rows("mask_minimized_stats", "bits", bits, n, ld_bits, G);
    if (((uintptr_t)feat_col | (uintptr_t)feat_start | (uintptr_t)feat_end) & 3)
      throw Gm2Error("mask_minimized_stats: the feature tables must be 4-B aligned");
    if (F && (!feat_col || !feat_start || !feat_end)) throw Gm2Error("mask_minimized_stats: null feature table");
    if (((uintptr_t)removed_bp | (uintptr_t)signature) & 7)
      throw Gm2Error("mask_minimized_stats: removed_bp and signature must be 8-B aligned");
    if ((uintptr_t)genes_removed & 3) throw Gm2Error("mask_minimized_stats: genes_removed must be 4-B aligned");
    if (n == 0) return;
    if (!removed_bp || !genes_removed || !signature) throw Gm2Error("mask_minimized_stats: null output");
    if (F == 0) {  // (no feature: nothing is removed)
      HIP_OK(hipMemsetAsync(removed_bp, 0, (size_t)n * 8, (hipStream_t)stream));
      HIP_OK(hipMemsetAsync(genes_removed, 0, (size_t)n * 4, (hipStream_t)stream));
      HIP_OK(hipMemsetAsync(signature, 0, (size_t)n * 8, (hipStream_t)stream));
      return;
    }
    launch_minimized_stats(bits, n, ld_bits, G, feat_col, feat_start, feat_end, F, removed_bp, genes_removed, signature,
                           (hipStream_t)stream);
  });
}

namespace {
constexpr int64_t kSearchMaxK = 65536, kSearchMaxN = (int64_t)1 << 20, kSearchMaxG = (int64_t)1 << 23;
constexpr int64_t kSearchMaxIndex = (int64_t)1 << 40;

void check_search_k(const char* what, int64_t K) {
  if (K < 1 || K > kSearchMaxK) throw Gm2Error("%s: K %lld outside [1, 65536]", what, (long long)K);
}
void check_search_genes(const char* what, int64_t G, int64_t n_groups) {
  if (G < 1 || G >= kSearchMaxG) throw Gm2Error("%s: G %lld outside [1, 2^23)", what, (long long)G);
  if (n_groups < 0 || n_groups > 0x7ffffffe) throw Gm2Error("%s: n_groups %lld outside [0, 2^31 - 1)", what, (long long)n_groups);
}
// the arrays of one state: all there, aligned, the rows pitched to cover G
void check_search_state(const char* what, const char* name, const gm2_search_state* st, int64_t G) {
  if (!st) throw Gm2Error("%s: null %s", what, name);
  check_search_k(what, st->K);
  if (!st->keys || !st->hashes || !st->essential || !st->rows || !st->count || !st->totals || !st->size_hist ||
      !st->ess_hist || !st->error)
    throw Gm2Error("%s: %s has a null array", what, name);
  if (((uintptr_t)st->keys | (uintptr_t)st->hashes | (uintptr_t)st->totals | (uintptr_t)st->size_hist |
       (uintptr_t)st->ess_hist) & 7)
    throw Gm2Error("%s: the 64-bit arrays of %s must be 8-B aligned", what, name);
  if (((uintptr_t)st->essential | (uintptr_t)st->count | (uintptr_t)st->error | (uintptr_t)st->z) & 3)
    throw Gm2Error("%s: the 32-bit arrays of %s must be 4-B aligned", what, name);
  if (st->ld_rows <= 0 || (st->ld_rows & 15) || st->ld_rows * 8 < G)
    throw Gm2Error("%s: row pitch of %s (%lld) must be a multiple of 16 bytes covering G = %lld bits", what, name,
                   (long long)st->ld_rows, (long long)G);
  if ((uintptr_t)st->rows & 15) throw Gm2Error("%s: rows of %s must be 16-B aligned", what, name);
  if (st->z && (st->L < 1 || st->ldz < st->L))
    throw Gm2Error("%s: z of %s needs 1 <= L (%lld) <= ldz (%lld)", what, name, (long long)st->L, (long long)st->ldz);
}
// the two winner buffers of a fold: the same geometry, different memory
void check_search_pair(const char* what, const gm2_search_state* in, const gm2_search_state* out, int64_t G) {
  check_search_state(what, "state_in", in, G);
  check_search_state(what, "state_out", out, G);
  if (in == out || in->keys == out->keys || in->hashes == out->hashes || in->essential == out->essential ||
      in->rows == out->rows || in->count == out->count || (in->z && in->z == out->z))
    throw Gm2Error("%s: state_in and state_out must be two different winner buffers", what);
  if (in->K != out->K || !in->z != !out->z || (in->z && in->L != out->L))
    throw Gm2Error("%s: state_in and state_out differ in K, L or in having z", what);
}
}  // namespace

int gm2_search_scratch_size(int64_t n_max, int64_t K, size_t* bytes) {
  return guarded([&] {
    if (!bytes) throw Gm2Error("search_scratch_size: null bytes");
    check_search_k("search_scratch_size", K);
    if (n_max < 0 || n_max > kSearchMaxN)
      throw Gm2Error("search_scratch_size: n_max %lld outside [0, 2^20]", (long long)n_max);
    *bytes = search_scratch_bytes(n_max, K);
  });
}

int gm2_search_init(const gm2_search_state* state, int64_t G, int64_t n_groups, void* stream) {
  return guarded([&] {
    check_search_genes("search_init", G, n_groups);
    check_search_state("search_init", "state", state, G);
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(hipMemsetAsync(state->count, 0, 4, s));
    HIP_OK(hipMemsetAsync(state->error, 0, 4, s));
    HIP_OK(hipMemsetAsync(state->totals, 0, 16, s));
    HIP_OK(hipMemsetAsync(state->size_hist, 0, (size_t)(G + 1) * 8, s));
    HIP_OK(hipMemsetAsync(state->ess_hist, 0, (size_t)(n_groups + 1) * 8, s));
  });
}

int gm2_search_push(const gm2_search_state* state_in, const gm2_search_state* state_out, void* scratch,
                    size_t scratch_bytes, const uint8_t* bits, int64_t n, int64_t ld_bits, int64_t G, const float* z,
                    int64_t ldz, int64_t base_index, const int32_t* group_offsets, int64_t n_groups,
                    const int32_t* positions, int64_t min_groups, void* stream) {
  return guarded([&] {
    check_search_genes("search_push", G, n_groups);
    check_search_pair("search_push", state_in, state_out, G);
    if (n > kSearchMaxN) throw Gm2Error("search_push: n %lld outside [0, 2^20]", (long long)n);
    check_bit_rows("search_push", "bits", bits, n, ld_bits, G);
    if (base_index < 0 || base_index > kSearchMaxIndex - n)
      throw Gm2Error("search_push: base index %lld outside [0, 2^40 - n]", (long long)base_index);
    if (min_groups < 0) throw Gm2Error("search_push: negative min_groups (%lld)", (long long)min_groups);
    if (n_groups && (!group_offsets || !positions)) throw Gm2Error("search_push: null group table with n_groups > 0");
    if (((uintptr_t)group_offsets | (uintptr_t)positions | (uintptr_t)z) & 3)
      throw Gm2Error("search_push: the group tables and z must be 4-B aligned");
    if (n == 0) return;
    if (!z != !state_in->z) throw Gm2Error("search_push: z is required exactly when the state keeps z");
    if (z && ldz < state_in->L) throw Gm2Error("search_push: ldz %lld < L %lld", (long long)ldz, (long long)state_in->L);
    if (!scratch || ((uintptr_t)scratch & 255)) throw Gm2Error("search_push: scratch must be 256-B aligned");
    if (search_scratch_bytes(n, state_in->K) > scratch_bytes)
      throw Gm2Error("search_push: scratch of %zu bytes, %zu needed (gm2_search_scratch_size)", scratch_bytes,
                     search_scratch_bytes(n, state_in->K));
    launch_search_push(*state_in, *state_out, scratch, bits, n, ld_bits, G, z, ldz, base_index, group_offsets, n_groups,
                       positions, min_groups, (hipStream_t)stream);
  });
}

int gm2_search_merge(const gm2_search_state* state_in, const gm2_search_state* state_out, void* scratch,
                     size_t scratch_bytes, const gm2_search_state* other, int64_t G, int64_t n_groups, void* stream) {
  return guarded([&] {
    check_search_genes("search_merge", G, n_groups);
    check_search_pair("search_merge", state_in, state_out, G);
    check_search_state("search_merge", "other", other, G);
    if (!other->z != !state_in->z || (other->z && other->L != state_in->L))
      throw Gm2Error("search_merge: other differs from the state in L or in having z");
    if (other->keys == state_in->keys || other->keys == state_out->keys || other->totals == state_out->totals)
      throw Gm2Error("search_merge: other must not share arrays with the state");
    if (!scratch || ((uintptr_t)scratch & 255)) throw Gm2Error("search_merge: scratch must be 256-B aligned");
    if (search_scratch_bytes(other->K, state_in->K) > scratch_bytes)
      throw Gm2Error("search_merge: scratch of %zu bytes, %zu needed (gm2_search_scratch_size)", scratch_bytes,
                     search_scratch_bytes(other->K, state_in->K));
    launch_search_merge(*state_in, *state_out, scratch, *other, G, n_groups, (hipStream_t)stream);
  });
}

int gm2_decode_bits(const gm2_dims* d, const float* params, const float* bn_running, const float* z, int64_t n,
                    uint8_t* bits, int64_t ld_bits, float* probs, int64_t ld_probs, void* ws, void* stream) {
  MaskOut o;
  o.bits = bits, o.ldb = ld_bits, o.probs = probs, o.ldpr = ld_probs;
  return decode_rows(d, params, bn_running, z, n, o, true, ws, stream);
}

int gm2_recon_counts(const gm2_dims* d, int prec, const gm2_batch* batch, const float* params, const float* bn_running,
                     float threshold, int32_t* counts, void* ws, void* stream) {
  return with_ws_joined(ws, stream, [&](WsState& st) {
    const Layout lo = make_layout(d, prec);
    drop_stage(st, (hipStream_t)stream);  // these write input slot 0
    if (!batch->eps) throw Gm2Error("recon_counts: eps required (model(x) samples z)");
    if (!counts) throw Gm2Error("recon_counts: counts required");
    HIP_OK(hipMemsetAsync(counts, 0, (size_t)batch->n * 3 * 4, (hipStream_t)stream));
    float* bn = const_cast<float*>(bn_running);  // eval mode never writes running stats
    by_precision(lo.prec, [&](auto tag) {
      using T = decltype(tag);
      Ctx<T> c(lo, ws, stream, st);
      FwdCall fw;
      fw.counts = counts, fw.thr = threshold;
      forward<T>(c, batch, params, bn, step_plan<T>(c, (int)batch->n), fw);
    });
  });
}

int gm2_encode(const gm2_dims* d, int prec, const gm2_batch* batch, const float* params, const float* bn_running,
               float* mu, float* logvar, void* ws, void* stream) {
  return with_ws_joined(ws, stream, [&](WsState& st) {
    const Layout lo = make_layout(d, prec);
    drop_stage(st, (hipStream_t)stream);  // these write input slot 0
    gm2_batch b = *batch;
    b.eps = nullptr;  // (mu and logvar alone: no z is drawn)
    by_precision(lo.prec, [&](auto tag) {
      using T = decltype(tag);
      Ctx<T> c(lo, ws, stream, st);
      const int B = (int)b.n;
      if (B <= 0 || B > c.d.Bm) throw Gm2Error("encode rows outside (0, batch_max]");
      check_batch_data(&b, c.d, "encode");
      const BnPass p{params, const_cast<float*>(bn_running), B, (int)round_up(B, kTile)};
      encoder_half<T>(c, &b, p, X3Plan{}, false);
      copy_heads<T>(c, B, mu, logvar);
    });
  });
}

int gm2_gemm(int prec, int pk, int qk, const void* P, int64_t ldp, const void* Q, int64_t ldq, float* C, int64_t ldc,
             int64_t M, int64_t N, int64_t K, int splits, float* slab_ws, void* stream) {
  return guarded([&] {
    // one launch into C, or split-K slabs in slab_ws column-summed into C ([S][M * ldc] as rows)
    auto run = [&](const auto& g, bool s3) {
      const hipStream_t s = (hipStream_t)stream;
      if (splits < 0) splits = plan_gemm(g).splits;  // the hot path's own tile / split-K plan
      if (splits > 1 && !slab_ws) throw Gm2Error("gemm: split-K needs slab_ws");
      const int S = gemm_store(g, s3, std::max(splits, 1), splits > 1 ? slab_ws : C, nullptr, 0, ldc,
                               splits > 1 ? M * ldc : 0, s);
      if (splits > 1) launch_colsum(slab_ws, S, M * ldc, M * ldc, C, nullptr, 0, s);
    };
    const int pk1 = pk ? 1 : 0, qk1 = qk ? 1 : 0;
    if (prec == GM2_F32) {
      run(GemmArgs<float>{(const float*)P, ldp, (const float*)Q, ldq, (int)M, (int)N, (int)K, (int)round_up(M, kTile),
                          (int)round_up(N, kTile), 0, pk1, qk1}, false);
    } else if (prec == GM2_BF16) {
      run(GemmArgs<bf16_t>{(const bf16_t*)P, ldp, (const bf16_t*)Q, ldq, (int)M, (int)N, (int)K,
                           (int)round_up(M, kTile), (int)round_up(N, kTile), 0, pk1, qk1}, false);
    } else if (prec == GM2_BF16X3) {  // operands from gm2_split_operand, K the real K
      if (K <= 0 || K % 32) throw Gm2Error("gemm (bf16x3): K %lld must be a positive multiple of 32", (long long)K);
      run(GemmArgs<bf16_t>{(const bf16_t*)P, ldp, (const bf16_t*)Q, ldq, (int)M, (int)N, (int)(2 * K),
                           (int)round_up(M, 2 * kTile), (int)round_up(N, 2 * kTile), 0, pk1, qk1}, true);
    } else {
      throw Gm2Error("bad precision");
    }
  });
}

int gm2_split_operand(const float* X, int64_t ldx, int64_t rows, int64_t K, int kmajor, uint16_t* out, int64_t ldo,
                      void* stream) {
  return guarded([&] {
    if (!X || !out || rows <= 0 || K <= 0 || K % 32 || rows > INT32_MAX - 256 || K > INT32_MAX / 2)
      throw Gm2Error("split operand: rows %lld, K %lld (a positive multiple of 32)", (long long)rows, (long long)K);
    const int rp = (int)round_up(rows, 2 * kTile);
    if (kmajor) launch_split_kmajor(X, ldx, (int)rows, (int)K, rp, (int)K, out, ldo, 0, nullptr, 0, (hipStream_t)stream);
    else launch_split_trans(X, ldx, (int)rows, (int)K, rp, out, ldo, (hipStream_t)stream);
  });
}

int gm2_forward(const gm2_dims* d, int prec, const gm2_batch* batch, const float* params, float* bn_running,
                int train, float* probs, int64_t ld_probs, float* mu, float* logvar, void* ws, void* stream) {
  return with_ws_joined(ws, stream, [&](WsState& st) {
    const Layout lo = make_layout(d, prec);
    drop_stage(st, (hipStream_t)stream);  // these write input slot 0
    if (!probs || ld_probs < lo.d.G) throw Gm2Error("forward: probs required, ld_probs >= G");
    if (!batch->eps) throw Gm2Error("forward: eps required (model.py:102 draws it)");
    by_precision(lo.prec, [&](auto tag) {
      using T = decltype(tag);
      Ctx<T> c(lo, ws, stream, st);
      FwdCall fw;
      fw.train = train, fw.probs = probs, fw.ld_probs = ld_probs;
      forward<T>(c, batch, params, bn_running, step_plan<T>(c, (int)batch->n), fw);
      copy_heads<T>(c, batch->n, mu, logvar);
    });
  });
}

int gm2_backward_outputs(const gm2_dims* d, int prec, const gm2_batch* batch, const float* params, int train,
                         const float* probs, int64_t ld_probs, const float* dprobs, const float* dmu,
                         const float* dlogvar, float* grads, void* ws, void* stream) {
  return with_ws_joined(ws, stream, [&](WsState& st) {
    const Layout lo = make_layout(d, prec);
    drop_stage(st, (hipStream_t)stream);  // these write input slot 0
    if (!probs || !dprobs || ld_probs < lo.d.G) throw Gm2Error("backward_outputs: probs / dprobs required");
    by_precision(lo.prec, [&](auto tag) {
      using T = decltype(tag);
      Ctx<T> c(lo, ws, stream, st);
      const Dims& dd = c.d;
      const int B = (int)batch->n, Bp = (int)round_up(B, kTile);
      if (B <= 0 || B > dd.Bm) throw Gm2Error("backward_outputs: rows outside (0, batch_max]");
      launch_sigmoid_bwd<T>(probs, dprobs, ld_probs, B, Bp, (int)dd.G, (int)dd.Gp, c.t(lo.dL), dd.Gp, c.f(lo.colpart),
                            c.s);
      launch_colsum(c.f(lo.colpart), Bp / 64, dd.Gp, dd.G, grads + dd.off[D9B], nullptr, 0, c.s);
      // the fused loss terms are absent here: beta = 0 in a private scalar block
      float* scal0 = c.f(lo.scal0);
      HIP_OK(hipMemsetAsync(scal0, 0, GM2_NUM_SCALARS * 4, c.s));
      BwdCall bw;
      bw.dmu_ext = dmu, bw.dlv_ext = dlogvar, bw.train = train;
      backward<T>(c, batch, params, grads, scal0, step_plan<T>(c, B), bw);
    });
  });
}

int gm2_reparameterize(int64_t n, const float* mu, const float* logvar, const float* eps, float* z,
                       const float* dz, float* dmu, float* dlogvar, void* stream) {
  return guarded([&] {
    if (!mu || !logvar || !eps || (!z && !dz) || (dz && (!dmu || !dlogvar)))
      throw Gm2Error("reparameterize: bad pointers");
    if (n < 0) throw Gm2Error("reparameterize: negative n %lld", (long long)n);
    launch_reparameterize(n, mu, logvar, eps, z, dz, dmu, dlogvar, (hipStream_t)stream);
  });
}

int gm2_exchange_pack(const float* x, int64_t n, uint16_t* out, int64_t n_pad, void* stream) {
  return guarded([&] { launch_exchange_pack(x, n, (bf16_t*)out, n_pad, (hipStream_t)stream); });
}

int gm2_exchange_ranksum(const uint16_t* parts, int world, int64_t chunk, uint16_t* out, void* stream) {
  return guarded([&] { launch_exchange_ranksum((const bf16_t*)parts, world, chunk, (bf16_t*)out, (hipStream_t)stream); });
}

int gm2_exchange_unpack(const uint16_t* in, int64_t n, float* x, void* stream) {
  return guarded([&] { launch_exchange_unpack((const bf16_t*)in, n, x, (hipStream_t)stream); });
}

int gm2_grad_bucket_bounds(const gm2_dims* d, int64_t* lo_hi) {
  return guarded([&] { bucket_bounds(make_dims(d), lo_hi); });
}

int gm2_wait_grad_bucket(void* ws, int bucket, void* stream) {
  return with_ws(ws, [&](WsState& st) {
    if (bucket < 0 || bucket >= GM2_GRAD_BUCKETS) throw Gm2Error("bucket %d out of range", bucket);
    if (!st.recorded)
      throw Gm2Error("no gm2_train_fwd_bwd has recorded gradient buckets on this workspace (none has run, or "
                     "GM2_OPT_GRAD_BUCKETS is 0)");
    HIP_OK(hipStreamWaitEvent((hipStream_t)stream, st.bucket[st.bucket_ev[bucket]], 0));
  });
}

int gm2_set_option(int key, int value) {
  return guarded([&] { set_default_option(key, value); });
}

int gm2_get_option(int key, int* value) {
  return guarded([&] { *value = option_get(default_options(), key); });
}

int gm2_workspace_set_option(void* ws, int key, int value) {
  return guarded([&] { option_set(ws_state(ws).opt, key, value); });
}

int gm2_workspace_get_option(void* ws, int key, int* value) {
  return guarded([&] { *value = option_get(ws_state(ws).opt, key); });
}

int gm2_workspace_join(void* ws, void* stream) {
  return with_ws(ws, [&](WsState& st) { st.join((hipStream_t)stream); });
}

int gm2_workspace_set_collective(void* ws, gm2_allreduce_fn fn, void* user) {
  return guarded([&] {
    WsState& st = ws_state(ws);
    st.coll = fn, st.coll_user = user;
  });
}

int gm2_workspace_stat(void* ws, int key, int64_t* value) {
  return guarded([&] {
    if (!value) throw Gm2Error("null value");
    WsState& st = ws_state(ws);
    switch (key) {
      case GM2_STAT_SPLIT_DECODES:
      case GM2_STAT_EXACT_DECODES:
      case GM2_STAT_SPLIT_TILES:
      case GM2_STAT_EXACT_TILES:
      case GM2_STAT_BAND_ELEMENTS:
      case GM2_STAT_BAND_FLIPS:
      case GM2_STAT_BAND_OVERFLOW:
      case GM2_STAT_SINGLE_TILES:
      case GM2_STAT_OVERFLOW_TILES: {
        unsigned long long cum[8] = {}, ovf = 0;  // (the gated decodes' device counters: waits for the device)
        if (st.decode_cum) {
          HIP_OK(hipDeviceSynchronize());
          HIP_OK(hipMemcpy(cum, st.decode_cum, sizeof cum, hipMemcpyDeviceToHost));
          HIP_OK(hipMemcpy(&ovf, st.decode_ovf, sizeof ovf, hipMemcpyDeviceToHost));
        }
        switch (key) {
          case GM2_STAT_SPLIT_DECODES: *value = (int64_t)cum[5]; break;
          case GM2_STAT_EXACT_DECODES: *value = st.exact_decodes + (int64_t)cum[6]; break;
          case GM2_STAT_SPLIT_TILES: *value = (int64_t)cum[0]; break;
          case GM2_STAT_EXACT_TILES: *value = (int64_t)cum[1]; break;
          case GM2_STAT_BAND_ELEMENTS: *value = (int64_t)cum[2]; break;
          case GM2_STAT_BAND_FLIPS: *value = (int64_t)cum[3]; break;
          case GM2_STAT_SINGLE_TILES: *value = (int64_t)cum[7]; break;
          case GM2_STAT_OVERFLOW_TILES: *value = (int64_t)ovf; break;
          default: *value = (int64_t)cum[4]; break;
        }
        break;
      }
      case GM2_TSTAT_SPLIT_GEMMS: *value = st.x3_split; break;
      case GM2_TSTAT_EXACT_GEMMS: *value = st.x3_exact; break;
      default: throw Gm2Error("unknown statistic %d", key);
    }
  });
}

int gm2_workspace_release(void* ws) {
  bool dropped = false;
  const int rc = guarded([&] { dropped = ws_release(ws); });
  if (rc == 0 && dropped) {
    g_err = "gm2_workspace_release: a queued output-layer Adam update (GM2_OPT_DEFER_OUTPUT_ADAM) was discarded; "
            "call gm2_workspace_join before releasing to keep it";
    return 1;
  }
  return rc;
}

int gm2_timing_begin(int kernel_classes) {
  return guarded([&] { timing_begin(kernel_classes); });
}

int gm2_timing_end(double* total_ms, int64_t* launches) {
  return guarded([&] { timing_end(total_ms, launches); });
}

int gm2_timing_class(int kernel_class, double* total_ms, int64_t* launches) {
  return guarded([&] {
    if (!total_ms || !launches) throw Gm2Error("null output");
    timing_class(kernel_class, total_ms, launches);
  });
}

#ifdef GM2_DEBUG
// ---- debug build only (include/gm2_debug.h) ----
int gm2_debug_flags(unsigned* flags) {
  return guarded([&] {
    if (!flags) throw Gm2Error("null flags");
    *flags = dbg_take_kernels() | dbg_take_gemm_store() | dbg_take_gemm_recon() | dbg_take_gemm_mask() | dbg_take_masks() | dbg_take_search();
  });
}

int gm2_debug_check_layout(const gm2_dims* d, int precision, int64_t* n_regions, int64_t* total) {
  return guarded([&] {
    const Layout o = make_layout(d, precision);
    auto r = t_regions;
    std::sort(r.begin(), r.end());
    int64_t end = 0;
    for (const auto& x : r) {
      if (x.first % 256) throw Gm2Error("region at %lld not 256-B aligned", (long long)x.first);
      if (x.first < end) throw Gm2Error("region at %lld overlaps the previous one (ends %lld)", (long long)x.first, (long long)end);
      end = x.first + x.second;
      if (end > o.total) throw Gm2Error("region at %lld (+%lld) past the total %lld", (long long)x.first, (long long)x.second, (long long)o.total);
    }
    // every named offset of the layout is one of the regions
    const int64_t named[] = {o.sE0, o.sE1, o.sE2, o.sHD, o.sD0, o.sD1, o.sD2, o.sD3, o.X, o.XB, o.HD, o.Z, o.dL,
                             o.slabs, o.side_slabs, o.DA, o.dH, o.AT5, o.dYT0, o.bnpart, o.colpart, o.losspart,
                             o.klpart, o.gradpart, o.colbwd, o.nahdr, o.nasq, o.clip, o.scal0, o.X1, o.XB1, o.syncb,
                             o.s3a, o.s3w, o.s3rn, o.s3cn, o.s3ctl, o.s3band, o.s3tlist, o.s3tcount, o.s3a1, o.s3w1,
                             o.s3ovf, o.s3bits, o.adamscal, o.ridx, o.x3w0, o.x3w9k, o.x3w9m, o.x3xd, o.x3x, o.x3a5k,
                             o.x3a5m, o.x3dlk, o.x3dlm, o.x3dy0, o.x3rows};
    auto known = [&](int64_t off) {
      for (const auto& x : r)
        if (x.first == off) return true;
      return false;
    };
    for (int64_t off : named)
      if (!known(off)) throw Gm2Error("named offset %lld is not a region start", (long long)off);
    for (int i = 0; i < 6; ++i)
      if (!known(o.Y[i]) || !known(o.A[i]) || !known(o.save[i]) || !known(o.dY[i]))
        throw Gm2Error("layer %d offsets are not region starts", i);
    if (n_regions) *n_regions = (int64_t)r.size();
    if (total) *total = o.total;
  });
}
#endif

}  // extern "C"
