// AddressSanitizer driver of libgm2's host-side logic (race detection / sanitizers).
// Built by `build_native.py --variant asan`: every csrc/*.hip compiled -DGM2_DEBUG with ASan on the
// HOST code only (-Xarch_host -fsanitize=address), linked with this file into one executable. It
// needs no GPU and launches no kernel: it drives the C-ABI entry points whose work is host
// arithmetic -- dims and parameter offsets, the workspace layout (gm2_debug_check_layout: alignment,
// overlap, bounds of every region), resident-operand layouts, gradient buckets, the option tables
// (every key, valid and invalid values, process defaults vs per-workspace state), the GEMM launch
// geometry (csrc/gemm_plan.hpp: plans, K-slices, capped grids, slab capacity), and the error
// paths of every entry point given null / inconsistent arguments or an unknown workspace -- so any
// heap / stack / global overflow or use-after-free in that code aborts the run with an ASan report.
// Exit code 0 = every check passed and ASan saw nothing. tests/test_asan_cpu.py runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gm2.h"
#include "../../include/gm2_debug.h"
#include "gm2_kernels.hpp"  // csrc/: plan_gemm<T> and, through gemm_plan.hpp, the launch-geometry rules

static int g_fail = 0;
#define CHECK(c, ...)                                     \
  do {                                                    \
    if (!(c)) {                                           \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                  \
      std::fprintf(stderr, "\n");                         \
      ++g_fail;                                           \
    }                                                     \
  } while (0)

// a call that must fail with a message containing `what`
static void expect_error(int rc, const char* what, const char* ctx) {
  CHECK(rc != 0, "%s: expected an error", ctx);
  const char* e = gm2_last_error();
  CHECK(e && std::strstr(e, what), "%s: error '%s' lacks '%s'", ctx, e ? e : "(null)", what);
}

static void dims_and_layouts() {
  const int64_t Gs[] = {1, 2, 127, 128, 129, 255, 256, 257, 20000, 55039};
  const int64_t Hs[] = {128, 256, 512, 1024};
  const int64_t Ls[] = {1, 2, 4, 8, 16, 32, 64, 128, 256};
  const int64_t Bs[] = {1, 2, 3, 63, 64, 127, 128, 129, 4096, 4097};
  int64_t checked = 0;
  for (int64_t G : Gs)
    for (int64_t H : Hs)
      for (int64_t L : Ls)
        for (int64_t B : Bs) {
          if (G * H > (int64_t)64 << 20 && B > 256 && H != 1024) continue;  // keep the sweep short
          gm2_dims d{G, H, L, B};
          int64_t n = 0;
          CHECK(gm2_param_count(&d, &n) == 0, "param_count %s", gm2_last_error());
          std::vector<int64_t> off(GM2_NUM_PARAMS + 1, -1);
          CHECK(gm2_param_offsets(&d, off.data()) == 0, "param_offsets");
          CHECK(off[0] == 0 && off[GM2_NUM_PARAMS] == n, "offsets span [0, %lld)", (long long)n);
          for (int i = 0; i < GM2_NUM_PARAMS; ++i) CHECK(off[i] < off[i + 1], "offsets ascend at %d", i);
          std::vector<int64_t> lh(2 * GM2_GRAD_BUCKETS, -1);
          CHECK(gm2_grad_bucket_bounds(&d, lh.data()) == 0, "bucket bounds");
          for (int b = 0; b < GM2_GRAD_BUCKETS; ++b)
            CHECK(0 <= lh[2 * b] && lh[2 * b] <= lh[2 * b + 1] && lh[2 * b + 1] <= n, "bucket %d in range", b);
          size_t f32_bytes = 0;
          for (int prec : {GM2_F32, GM2_BF16, GM2_BF16X3}) {
            size_t bytes = 0;
            CHECK(gm2_workspace_size(&d, prec, &bytes) == 0, "workspace_size %s", gm2_last_error());
            // (GM2_BF16X3: the GM2_F32 layout plus the split operand buffers)
            if (prec == GM2_F32) f32_bytes = bytes;
            if (prec == GM2_BF16X3) CHECK(bytes > f32_bytes, "bf16x3 workspace %zu vs f32 %zu", bytes, f32_bytes);
            int64_t nreg = 0, total = 0;
            const int rc = gm2_debug_check_layout(&d, prec, &nreg, &total);
            CHECK(rc == 0, "layout G=%lld H=%lld L=%lld B=%lld prec=%d: %s", (long long)G, (long long)H,
                  (long long)L, (long long)B, prec, gm2_last_error());
            CHECK((size_t)total == bytes && nreg > 50, "layout total %lld vs size %zu, %lld regions",
                  (long long)total, bytes, (long long)nreg);
            ++checked;
          }
        }
  std::printf("layouts checked: %lld\n", (long long)checked);
  // bad dims
  gm2_dims bad[] = {{0, 128, 8, 8}, {10, 100, 8, 8}, {10, 128, 3, 8}, {10, 128, 8, 0}, {-5, 128, 8, 8}};
  size_t bytes = 0;
  for (auto& d : bad) CHECK(gm2_workspace_size(&d, GM2_BF16, &bytes) != 0, "bad dims accepted");
  expect_error(gm2_workspace_size(nullptr, GM2_BF16, &bytes), "null dims", "null dims");
  gm2_dims d{100, 128, 8, 16};
  expect_error(gm2_workspace_size(&d, 7, &bytes), "precision", "bad precision");
  expect_error(gm2_workspace_size(&d, 3, &bytes), "bad precision", "precision 3");
  int64_t nreg = 0, total = 0;
  expect_error(gm2_debug_check_layout(&d, 3, &nreg, &total), "bad precision", "layout of precision 3");
  // resident layouts
  for (int64_t S : {1, 2, 63, 64, 10000})
    for (int64_t G : {1, 255, 256, 20000, 55039})
      for (int prec : {GM2_F32, GM2_BF16}) {
        int64_t ld = 0, ldb = 0, rows = 0;
        size_t nb = 0, nbb = 0;
        CHECK(gm2_resident_layout(S, G, prec, &ld, &ldb, &rows, &nb, &nbb) == 0, "resident layout %s",
              gm2_last_error());
        CHECK(ld >= G && ld % 256 == 0 && ldb * 32 == ld && rows >= S + 1 && rows % 64 == 0, "resident shape");
        CHECK(nb == (size_t)(rows * ld * (prec == GM2_F32 ? 4 : 2)) && nbb == (size_t)(rows * ldb * 4),
              "resident bytes");
      }
  for (int64_t G : {1, 8, 9, 127, 128, 55039}) CHECK(gm2_packed_row_bytes(G) >= (G + 7) / 8, "packed row bytes");
}

static const int kKeys[] = {GM2_OPT_GEMM_PP,      GM2_OPT_SIDE_STREAM,  GM2_OPT_RECON_TILE,        GM2_OPT_SMALL_SPLIT,
                            GM2_OPT_BN_EPILOGUE,  GM2_OPT_SMALL_WAVES,  GM2_OPT_INPUT_CHUNKS,      GM2_OPT_GRID_CAP,
                            GM2_OPT_SYNC_BN,      GM2_OPT_DEFER_OUTPUT_ADAM, GM2_OPT_GRAD_BUCKETS, GM2_OPT_SAMPLE_SPLIT,
                            GM2_OPT_SAMPLE_SINGLE, GM2_OPT_SAMPLE_BAND_CAP, GM2_OPT_SAMPLE_SINGLE_BOUND,
                            GM2_OPT_TRAIN_SPLIT};

static void options() {
  std::vector<int> saved;
  for (int k : kKeys) {
    int v = -99;
    CHECK(gm2_get_option(k, &v) == 0, "get option %d", k);
    saved.push_back(v);
  }
  // every key: a sweep of values; accepted ones read back as set (or clamped / booleanised)
  const int probe[] = {-100000, -2, -1, 0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 64, 128, 256, 4096, 4097, 1 << 30};
  int accepted = 0, rejected = 0;
  for (int k : kKeys)
    for (int v : probe) {
      int before = 0;
      gm2_get_option(k, &before);
      if (gm2_set_option(k, v) == 0) {
        int got = -12345;
        CHECK(gm2_get_option(k, &got) == 0, "get after set");
        CHECK(got != -12345, "option %d read back", k);
        ++accepted;
      } else {
        int got = -12345;
        gm2_get_option(k, &got);
        CHECK(got == before, "a rejected set of option %d changed it (%d -> %d)", k, before, got);
        ++rejected;
      }
    }
  std::printf("option values accepted %d, rejected %d\n", accepted, rejected);
  for (int bad : {0, -1, 23, 1000}) {
    int v = 0;
    expect_error(gm2_set_option(bad, 1), "unknown option", "set unknown key");
    expect_error(gm2_get_option(bad, &v), "unknown option", "get unknown key");
  }
  // GM2_OPT_TRAIN_SPLIT: default 1, 0 and 1 accepted, anything else refused and the value kept
  {
    int v = -1;
    gm2_set_option(GM2_OPT_TRAIN_SPLIT, 1);
    CHECK(gm2_set_option(GM2_OPT_TRAIN_SPLIT, 0) == 0 && gm2_get_option(GM2_OPT_TRAIN_SPLIT, &v) == 0 && v == 0,
          "train split off");
    for (int bad : {-1, 2, 3, 256})
      expect_error(gm2_set_option(GM2_OPT_TRAIN_SPLIT, bad), "train split", "train split value");
    CHECK(gm2_get_option(GM2_OPT_TRAIN_SPLIT, &v) == 0 && v == 0, "a refused train split value changed it");
    CHECK(gm2_set_option(GM2_OPT_TRAIN_SPLIT, 1) == 0 && gm2_get_option(GM2_OPT_TRAIN_SPLIT, &v) == 0 && v == 1,
          "train split on");
  }
  for (size_t i = 0; i < saved.size(); ++i) gm2_set_option(kKeys[i], saved[i]);
  // per-workspace entry points on a workspace libgm2 never initialised
  char host_buf[64];
  void* ws = host_buf;
  int v = 0;
  expect_error(gm2_workspace_set_option(ws, GM2_OPT_GRID_CAP, 1), "not initialised", "ws set");
  expect_error(gm2_workspace_get_option(ws, GM2_OPT_GRID_CAP, &v), "not initialised", "ws get");
  expect_error(gm2_wait_grad_bucket(ws, 0, nullptr), "not initialised", "wait bucket");
  expect_error(gm2_workspace_join(ws, nullptr), "not initialised", "join");
  expect_error(gm2_workspace_set_collective(ws, nullptr, nullptr), "not initialised", "collective");
  int64_t stat = 0;
  expect_error(gm2_workspace_stat(ws, GM2_STAT_SPLIT_DECODES, &stat), "not initialised", "stat");
  expect_error(gm2_workspace_stat(ws, GM2_TSTAT_SPLIT_GEMMS, &stat), "not initialised", "train stat");
  CHECK(gm2_workspace_release(ws) == 0, "release of unknown state is a no-op");
}

// entry points that reach the device: with no GPU (or with arguments refused before any device
// work) each returns an error and leaves nothing behind
static void error_paths() {
  gm2_dims d{300, 128, 8, 64};
  size_t bytes = 0;
  gm2_workspace_size(&d, GM2_BF16, &bytes);
  std::vector<char> host(1 << 16);
  int rc = gm2_workspace_init(&d, GM2_BF16, host.data(), 16, nullptr);  // far too small
  CHECK(rc != 0, "init with a too-small workspace accepted");
  rc = gm2_workspace_init(&d, GM2_BF16, nullptr, bytes, nullptr);
  CHECK(rc != 0, "init with a null workspace accepted");
  rc = gm2_workspace_init(nullptr, GM2_BF16, host.data(), bytes, nullptr);
  CHECK(rc != 0, "init with null dims accepted");
  gm2_batch b{};
  float f = 0.f;
  double loss[GM2_LOSS_SLOTS] = {};
  CHECK(gm2_train_fwd_bwd(&d, GM2_BF16, nullptr, &f, &f, &f, &f, loss, host.data(), nullptr) != 0, "null batch");
  CHECK(gm2_train_fwd_bwd(&d, GM2_BF16, &b, &f, &f, &f, &f, loss, host.data(), nullptr) != 0, "empty batch");
  CHECK(gm2_eval_forward(&d, GM2_BF16, &b, &f, &f, &f, loss, host.data(), nullptr) != 0, "eval empty batch");
  CHECK(gm2_grad_norm(nullptr, GM2_BF16, &f, &f, &f, loss, host.data(), nullptr) != 0, "grad_norm null dims");
  CHECK(gm2_adam_step(nullptr, GM2_BF16, &f, &f, &f, &f, &f, host.data(), nullptr) != 0, "adam null dims");
  CHECK(gm2_sync_shadows(&d, 5, &f, host.data(), nullptr) != 0, "sync_shadows bad precision");
  CHECK(gm2_train_fwd_bwd(&d, GM2_BF16X3, &b, &f, &f, &f, &f, loss, host.data(), nullptr) != 0, "bf16x3 empty batch");
  CHECK(gm2_eval_forward(&d, GM2_BF16X3, &b, &f, &f, &f, loss, host.data(), nullptr) != 0, "bf16x3 eval empty batch");
  uint16_t h16 = 0;
  CHECK(gm2_split_operand(nullptr, 32, 4, 32, 1, &h16, 64, nullptr) != 0, "split operand null input");
  CHECK(gm2_split_operand(&f, 32, 4, 33, 1, &h16, 64, nullptr) != 0, "split operand K not a multiple of 32");
  CHECK(gm2_split_operand(&f, 32, 0, 32, 0, &h16, 256, nullptr) != 0, "split operand no rows");
  CHECK(gm2_gemm(GM2_BF16X3, 1, 1, &h16, 64, &h16, 64, &f, 4, 4, 4, 33, 1, nullptr, nullptr) != 0, "bf16x3 gemm K not a multiple of 32");
  CHECK(gm2_gemm(3, 1, 1, &h16, 64, &h16, 64, &f, 4, 4, 4, 32, 1, nullptr, nullptr) != 0, "gemm precision 3");
  int64_t ld = 0, ldb = 0, rows = 0;
  size_t nb = 0, nbb = 0;
  CHECK(gm2_resident_layout(-1, 10, GM2_BF16, &ld, &ldb, &rows, &nb, &nbb) != 0, "negative S");
  CHECK(gm2_resident_layout(10, 0, GM2_BF16, &ld, &ldb, &rows, &nb, &nbb) != 0, "zero G");
  CHECK(gm2_reparameterize(-1, &f, &f, &f, &f, nullptr, nullptr, nullptr, nullptr) != 0, "negative n");
  // bit-row cross products: every refusal is host-side, zero rows return before any launch
  alignas(16) static uint8_t rows_a[64], rows_b[64];
  int32_t co[8];
  int64_t best[4];
  expect_error(gm2_mask_cooccur(rows_a, -1, 16, rows_b, 2, 16, 100, co, 2, nullptr), "negative", "cooccur na < 0");
  expect_error(gm2_mask_cooccur(rows_a, 2, 16, rows_b, 2, 16, 0, co, 2, nullptr), "G", "cooccur G = 0");
  expect_error(gm2_mask_cooccur(rows_a, 2, 24, rows_b, 2, 16, 100, co, 2, nullptr), "pitch", "cooccur lda % 16");
  expect_error(gm2_mask_cooccur(rows_a, 2, 16, rows_b, 2, 16, 129, co, 2, nullptr), "pitch", "cooccur pitch < G bits");
  expect_error(gm2_mask_cooccur(rows_a + 8, 2, 16, rows_b, 2, 16, 100, co, 2, nullptr), "aligned", "cooccur misaligned a");
  expect_error(gm2_mask_cooccur(rows_a, 2, 16, rows_b, 2, 16, 100, co, 1, nullptr), "ldo", "cooccur ldo < nb");
  CHECK(gm2_mask_cooccur(rows_a, 0, 16, rows_b, 2, 16, 100, co, 2, nullptr) == 0, "cooccur with no a rows");
  CHECK(gm2_mask_cooccur(rows_a, 2, 16, rows_b, 0, 16, 100, co, 0, nullptr) == 0, "cooccur with no b rows");
  expect_error(gm2_mask_nearest(rows_a, 2, 16, rows_b, 0, 16, 100, best, nullptr), "nr", "nearest nr = 0");
  expect_error(gm2_mask_nearest(rows_a, 2, 16, rows_b + 4, 2, 16, 100, best, nullptr), "aligned", "nearest misaligned ref");
  expect_error(gm2_mask_nearest(rows_a, 2, 16, rows_b, -2, 16, 100, best, nullptr), "negative", "nearest nr < 0");
  CHECK(gm2_mask_nearest(rows_a, 0, 16, rows_b, 2, 16, 100, best, nullptr) == 0, "nearest with no queries");
  // per-gene counts: the same vocabulary; no rows to add into a kept vector returns before any device call
  int64_t gc[128];
  int32_t idx[2] = {0, 1};
  expect_error(gm2_mask_gene_counts(rows_a, 2, 16, 100, nullptr, -1, gc, 0, nullptr), "negative", "gene_counts n < 0");
  expect_error(gm2_mask_gene_counts(rows_a, -2, 16, 100, nullptr, 0, gc, 0, nullptr), "negative", "gene_counts n_rows < 0");
  expect_error(gm2_mask_gene_counts(rows_a, 2, 16, 100, nullptr, 3, gc, 0, nullptr), "n_rows", "gene_counts n > n_rows");
  expect_error(gm2_mask_gene_counts(rows_a, 2, 16, 0, nullptr, 2, gc, 0, nullptr), "G", "gene_counts G = 0");
  expect_error(gm2_mask_gene_counts(rows_a, 2, 24, 100, nullptr, 2, gc, 0, nullptr), "pitch", "gene_counts pitch % 16");
  expect_error(gm2_mask_gene_counts(rows_a, 2, 16, 129, nullptr, 2, gc, 0, nullptr), "pitch", "gene_counts pitch < G bits");
  expect_error(gm2_mask_gene_counts(rows_a + 8, 2, 16, 100, nullptr, 2, gc, 0, nullptr), "aligned", "gene_counts misaligned bits");
  expect_error(gm2_mask_gene_counts(rows_a, 2, 16, 100, idx, 2, (int64_t*)((char*)gc + 4), 1, nullptr), "aligned",
               "gene_counts misaligned counts");
  expect_error(gm2_mask_gene_counts(rows_a, 2, 16, 100, idx, 2, nullptr, 1, nullptr), "null", "gene_counts null counts");
  CHECK(gm2_mask_gene_counts(rows_a, 2, 16, 100, nullptr, 0, gc, 1, nullptr) == 0, "gene_counts of no rows, accumulating");
  CHECK(gm2_mask_gene_counts(rows_a, 2, 16, 100, idx, 0, gc, 1, nullptr) == 0, "gene_counts of an empty list, accumulating");
  // bit transpose: 4 rows of 100 genes -> 100 rows of 4 bits; every refusal is host-side
  alignas(16) static uint8_t tr_in[4 * 16], tr_out[100 * 16];
  expect_error(gm2_mask_transpose(tr_in, -1, 16, 100, tr_out, 16, nullptr), "negative", "transpose n < 0");
  expect_error(gm2_mask_transpose(tr_in, 4, 16, 0, tr_out, 16, nullptr), "G", "transpose G = 0");
  expect_error(gm2_mask_transpose(tr_in, 4, 24, 100, tr_out, 16, nullptr), "pitch", "transpose ld_bits % 16");
  expect_error(gm2_mask_transpose(tr_in, 4, 16, 129, tr_out, 16, nullptr), "pitch", "transpose pitch < G bits");
  expect_error(gm2_mask_transpose(tr_in, 4, 16, 100, tr_out, 24, nullptr), "pitch", "transpose ld_out % 16");
  expect_error(gm2_mask_transpose(tr_in, 129, 16, 100, tr_out, 16, nullptr), "pitch", "transpose ld_out * 8 < n");
  expect_error(gm2_mask_transpose(tr_in + 8, 4, 16, 100, tr_out, 16, nullptr), "aligned", "transpose misaligned bits");
  expect_error(gm2_mask_transpose(tr_in, 4, 16, 100, tr_out + 4, 16, nullptr), "aligned", "transpose misaligned out");
  expect_error(gm2_mask_transpose(tr_in, 4, 16, 100, nullptr, 16, nullptr), "null", "transpose null out");
  expect_error(gm2_mask_transpose(tr_out, 4, 16, 100, tr_out + 48, 16, nullptr), "overlap", "transpose out inside bits");
  CHECK(gm2_mask_transpose(tr_in, 0, 16, 100, tr_out, 16, nullptr) == 0, "transpose of no rows");
  // minimized sizes: 2 rows of 100 genes, 3 features; every refusal is host-side
  int32_t ft[3] = {0, -1, -2};
  int64_t ms_bp[2];
  int32_t ms_gone[2];
  uint64_t ms_sig[2];
  expect_error(gm2_mask_minimized_stats(rows_a, -1, 16, 100, ft, ft, ft, 3, ms_bp, ms_gone, ms_sig, nullptr), "negative",
               "minimized_stats n < 0");
  expect_error(gm2_mask_minimized_stats(rows_a, 2, 16, 0, ft, ft, ft, 3, ms_bp, ms_gone, ms_sig, nullptr), "G",
               "minimized_stats G = 0");
  expect_error(gm2_mask_minimized_stats(rows_a, 2, 16, 100, ft, ft, ft, -1, ms_bp, ms_gone, ms_sig, nullptr), "F",
               "minimized_stats F < 0");
  expect_error(gm2_mask_minimized_stats(rows_a, 2, 24, 100, ft, ft, ft, 3, ms_bp, ms_gone, ms_sig, nullptr), "pitch",
               "minimized_stats pitch % 16");
  expect_error(gm2_mask_minimized_stats(rows_a, 2, 16, 129, ft, ft, ft, 3, ms_bp, ms_gone, ms_sig, nullptr), "pitch",
               "minimized_stats pitch < G bits");
  expect_error(gm2_mask_minimized_stats(rows_a + 8, 2, 16, 100, ft, ft, ft, 3, ms_bp, ms_gone, ms_sig, nullptr), "aligned",
               "minimized_stats misaligned bits");
  expect_error(gm2_mask_minimized_stats(rows_a, 2, 16, 100, (int32_t*)((char*)ft + 2), ft, ft, 3, ms_bp, ms_gone, ms_sig,
                                        nullptr), "aligned", "minimized_stats misaligned table");
  expect_error(gm2_mask_minimized_stats(rows_a, 2, 16, 100, ft, ft, ft, 3, (int64_t*)((char*)ms_bp + 4), ms_gone, ms_sig,
                                        nullptr), "aligned", "minimized_stats misaligned removed_bp");
  expect_error(gm2_mask_minimized_stats(rows_a, 2, 16, 100, ft, nullptr, ft, 3, ms_bp, ms_gone, ms_sig, nullptr), "null",
               "minimized_stats null table");
  expect_error(gm2_mask_minimized_stats(rows_a, 2, 16, 100, ft, ft, ft, 3, ms_bp, nullptr, ms_sig, nullptr), "null",
               "minimized_stats null output");
  CHECK(gm2_mask_minimized_stats(rows_a, 0, 16, 100, ft, ft, ft, 3, ms_bp, ms_gone, ms_sig, nullptr) == 0,
        "minimized_stats of no rows");
  CHECK(gm2_mask_minimized_stats(rows_a, 0, 16, 100, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == 0,
        "minimized_stats of no rows and no features");
  std::string last = gm2_last_error();
  CHECK(!last.empty(), "an error message is kept");
  unsigned flags = 1;
  CHECK(gm2_debug_flags(nullptr) != 0, "debug flags null");
  (void)flags;
}

// csrc/gemm_plan.hpp: every rule of the GEMM launch geometry against expected values (derived by
// hand from the rules as the launchers stated them before the header existed)
static void gemm_geometry() {
  using namespace gm2;
  // plan_gemm under the default options: the pure rule and the launchers' wrapper
  struct PlanRow {
    int esize, Mp, Np, K, tile, splits;
  };
  const PlanRow plans[] = {{2, 1024, 55040, 1024, 256, 1},  {2, 55040, 1024, 1024, 256, 1},
                           {2, 1024, 1024, 55040, 256, 16}, {4, 1024, 1024, 55040, 128, 4},
                           {2, 1024, 1024, 1024, 128, 2},   {4, 1024, 1024, 1024, 128, 4},
                           {2, 128, 1024, 55040, 128, 32},  {2, 2048, 1024, 1024, 128, 2},
                           {2, 4096, 1024, 1024, 128, 1}};
  for (const PlanRow& r : plans) {
    const GemmPlan p = plan_gemm_dims(r.esize, r.Mp, r.Np, r.K, 1);
    CHECK(p.tile == r.tile && p.splits == r.splits, "plan_gemm_dims(%d; %d, %d, %d) = {%d, %d}, expected {%d, %d}",
          r.esize, r.Mp, r.Np, r.K, p.tile, p.splits, r.tile, r.splits);
    GemmPlan w;
    if (r.esize == 2) {
      GemmArgs<bf16_t> g{nullptr, 0, nullptr, 0, r.Mp, r.Np, r.K, r.Mp, r.Np, 0};
      w = plan_gemm<bf16_t>(g);
    } else {
      GemmArgs<float> g{nullptr, 0, nullptr, 0, r.Mp, r.Np, r.K, r.Mp, r.Np, 0};
      w = plan_gemm<float>(g);
    }
    CHECK(w.tile == r.tile && w.splits == r.splits, "plan_gemm<%d B>(%d, %d, %d) = {%d, %d}, expected {%d, %d}",
          r.esize, r.Mp, r.Np, r.K, w.tile, w.splits, r.tile, r.splits);
  }
  // GM2_OPT_SMALL_SPLIT reaches the chip-filling short-K 128-tile plans only
  CHECK(plan_gemm_dims(2, 4096, 1024, 1024, 2).splits == 2 && plan_gemm_dims(2, 1024, 55040, 1024, 2).splits == 1,
        "small_split");
  struct SliceRow {
    int K, kt, want, kps, splits;
  };
  const SliceRow slices[] = {{55040, 64, 16, 3456, 16}, {55040, 64, 32, 1728, 32}, {55040, 32, 4, 13760, 4},
                             {2112, 64, 3, 704, 3},     {576, 64, 4, 192, 3},      {576, 32, 4, 160, 4},
                             {64, 64, 8, 64, 1}};
  for (const SliceRow& r : slices) {
    const KSlices k = k_slices(r.K, r.kt, r.want);
    CHECK(k.k_per_split == r.kps && k.splits == r.splits, "k_slices(%d, %d, %d) = {%d, %d}, expected {%d, %d}", r.K,
          r.kt, r.want, k.k_per_split, k.splits, r.kps, r.splits);
    // every slice whole K-tiles, together covering K, the last one not empty
    CHECK(k.k_per_split % r.kt == 0 && (int64_t)k.k_per_split * k.splits >= r.K &&
              (int64_t)k.k_per_split * (k.splits - 1) < r.K && k.splits <= std::max(r.want, 1),
          "k_slices(%d, %d, %d) does not cover K", r.K, r.kt, r.want);
  }
  const int grids[][4] = {{860, 256, 215, 860}, {256, 256, 256, 0}, {300, 256, 150, 300}, {100, 256, 100, 0}};
  for (const auto& r : grids) {
    const GridCap c = capped_grid(r[0], r[1]);
    CHECK(c.grid == r[2] && c.ntiles == r[3], "capped_grid(%d, %d) = {%d, %d}, expected {%d, %d}", r[0], r[1], c.grid,
          c.ntiles, r[2], r[3]);
  }
  static_assert(kMaxIdxRows == 8192, "the row-table cases below sit at this limit");
  CHECK(row_table_fits(8192, 64, 1), "row table: exactly kMaxIdxRows k-rows fit");
  CHECK(!row_table_fits(8256, 64, 1), "row table: one K-tile past kMaxIdxRows does not fit");
  CHECK(row_table_fits(16384, 64, 2), "row table: two slices of kMaxIdxRows fit");
  // slab capacity, into slabs: padded-row slabs, the plan's count clamped, none fitting an error
  const int64_t padded = slab_elems_padded(1024, 1024);
  CHECK(padded == (int64_t)1 << 20, "padded slab");
  CHECK(splits_into_slabs(16, padded, (int64_t)64 << 20) == 16, "into slabs, under capacity");
  CHECK(splits_into_slabs(16, padded, 16 * padded) == 16, "into slabs, at capacity");
  CHECK(splits_into_slabs(16, padded, 4 * padded + 5) == 4, "into slabs, over capacity: clamped");
  bool threw = false;
  try {
    splits_into_slabs(16, padded, padded - 1);
  } catch (const std::exception& e) {
    threw = std::strstr(e.what(), "slab capacity exceeded") != nullptr;
  }
  CHECK(threw, "into slabs, not one slab fits: an error");
  // into C: dense slabs (M x N rounded up to 4); over capacity the plain GEMMs take one pass, the
  // bf16x3 ones the slices that fit
  const int64_t dense = slab_elems_dense(999, 1001);
  CHECK(dense == 1000000, "dense slab");
  for (bool shrink : {false, true}) {
    CHECK(splits_into_c(16, dense, 16 * dense, shrink) == 16, "into C, at capacity (shrink %d)", (int)shrink);
    CHECK(splits_into_c(1, dense, 0, shrink) == 1, "into C, one pass needs no scratch (shrink %d)", (int)shrink);
  }
  CHECK(splits_into_c(16, dense, 16 * dense - 1, false) == 1, "into C, over capacity, plain: one pass");
  CHECK(splits_into_c(16, dense, 16 * dense - 1, true) == 15, "into C, over capacity, bf16x3: the slices that fit");
  CHECK(splits_into_c(16, dense, dense - 1, true) == 1, "into C, no slab fits, bf16x3: one pass");
}

int main() {
  CHECK(gm2_abi_version() == GM2_ABI_VERSION, "abi version");
  dims_and_layouts();
  options();
  gemm_geometry();
  error_paths();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("host_asan: all checks passed\n");
  return 0;
}
