// Streaming search for the smallest viable distinct genomes on the packed masks (gm2.h gm2_search_*):
// a device-resident running top-K with exact duplicate removal. The reference's answer to "a minimal
// genome" is focused sampling (main.py:351-370); this screens any number of decoded chunks and keeps the
// K smallest distinct rows that still carry their essential genes (count_essential_genes,
// utils/extras.py:49-87). One push folds a chunk of n packed rows into a state of at most K winners, as
// five stream-ordered launches behind one memset; nothing is allocated, nothing waits for another
// workgroup, nothing is read back:
//   score   one wave per row, every row byte read once with 16-byte loads: popcount (genome size), the
//           essential count by the whole-row form of masks.hip's k_count_groups_rows (an LDS bit mask of
//           the single-position groups, the other groups from the wave's staged row), and the 64-bit row
//           hash; the stream totals and both histograms with 64-bit integer atomics (a workgroup adds
//           each distinct value of its rows once, with its multiplicity)
//   insert  candidates = the state's winners + the chunk's viable rows, into an open-addressing hash set
//           in global memory (>= 2 x candidates slots, cleared per push): 64-bit CAS on the hash, then
//           atomicMin of the key on the slot; probing bounded by the table size, exhaustion -> error flag
//   mark    a candidate whose slot's minimum is not its own key is a later copy: key := all ones
//   select  one workgroup: MSB-first radix select (eight 8-bit passes, LDS histogram) of the K-th
//           smallest key, then the positions of the keys <= it; the winner count stays on the device
//   gather  one wave per winner: key, hash, essential count, packed row (16-byte copies) and z row from
//           the old state or the chunk into the new state (ping-pong)
// A merge runs the same path with another state's winners as the chunk.
#include "../../include/gm2.h"
#include "gm2_common.hpp"
#include "gm2_kernels.hpp"

namespace gm2 {

namespace {

constexpr unsigned long long kNoKey = ~0ull;   // a candidate that is not eligible; an empty table slot
constexpr int kSsRows = 64;                    // rows of a score workgroup (4 waves x 16)
constexpr unsigned long long kSsGolden = 0x9e3779b97f4a7c15ull;

__device__ __forceinline__ unsigned long long ss_mix(unsigned long long z) {  // the splitmix64 finalizer
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

__device__ __forceinline__ int ss_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ unsigned long long ss_wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// hist[v] += the rows of this workgroup with value v, one atomic per distinct value: the lowest row that
// holds a value adds its multiplicity (sizes and essential counts of neighbouring samples repeat, and
// 64 atomics on one address serialise at the memory side)
__device__ __forceinline__ void ss_hist_add(const int* __restrict__ vals, int rows, int t, int64_t bins,
                                            unsigned long long* __restrict__ hist) {
  if (t >= rows) return;
  const int v = vals[t];
  int mult = 0;
  bool first = true;
  for (int j = 0; j < rows; ++j) {
    const bool same = vals[j] == v;
    mult += same;
    first = first && !(same && j < t);
  }
  GM2_DBG(v >= 0 && v < bins, kDbgMaskPos);
  if (first && v >= 0 && v < bins) atomicAdd(&hist[v], (unsigned long long)mult);
}

// Per chunk row: key (size << 40 | base + row when viable, else all ones), hash, essential count; totals.
// LDS: [mask kb bytes][group list ngroups ints][4 staged rows of kb bytes], by mode:
//   use_mask  the single-position groups as a bit mask, the others (and a second group on a gene) listed
//   stage     each wave's row staged, the listed groups' byte reads go to LDS
// without use_mask (the tables do not fit 60 KB) every group is evaluated from global memory.
__global__ __launch_bounds__(256) void k_search_score(const uint8_t* __restrict__ bits, int n, int64_t ldb, int kb16,
                                                    int G, const int32_t* __restrict__ goff, int ngroups,
                                                    const int32_t* __restrict__ pos, int min_groups,
                                                    unsigned long long base, unsigned long long* __restrict__ ckey,
                                                    unsigned long long* __restrict__ chash, int32_t* __restrict__ cess,
                                                    unsigned long long* __restrict__ totals,
                                                    unsigned long long* __restrict__ size_hist,
                                                    unsigned long long* __restrict__ ess_hist, int use_mask, int stage) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ss_lds[];
  __shared__ int s_size[kSsRows], s_ess[kSsRows], s_ng;
  const int kb = kb16 * 16, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t* lmask = ss_lds;
  int* glist = (int*)(ss_lds + (use_mask ? kb / 4 : 0));
  uint8_t* wrow = (uint8_t*)ss_lds + (((size_t)(use_mask ? kb : 0) + (size_t)(use_mask ? ngroups : 0) * 4 + 15) & ~(size_t)15) +
                  (size_t)wave * kb;
  if (use_mask) {
    for (int i = threadIdx.x; i < kb / 4; i += 256) lmask[i] = 0u;
    if (threadIdx.x == 0) s_ng = 0;
    __syncthreads();
    for (int g = threadIdx.x; g < ngroups; g += 256) {
      const int k0 = goff[g], k1 = goff[g + 1];
      GM2_DBG(k0 >= 0 && k0 <= k1, kDbgMaskPos);
      if (k1 <= k0) continue;  // (an empty group never counts)
      if (k1 - k0 == 1) {
        const int p = pos[k0];
        GM2_DBG(p >= 0 && p < G, kDbgMaskPos);
        if (p < 0 || p >= G) continue;  // (never read: never set)
        const uint32_t bit = 1u << (p & 31);
        if (!(atomicOr(&lmask[p >> 5], bit) & bit)) continue;
      }
      const int slot = atomicAdd(&s_ng, 1);
      GM2_DBG(slot >= 0 && slot < ngroups, kDbgMaskPos);
      glist[slot] = g;
    }
    __syncthreads();
  }
  const int ng = use_mask ? s_ng : ngroups;
  const int row0 = blockIdx.x * kSsRows, r1 = min(n, row0 + kSsRows);
  for (int row = row0 + wave; row < r1; row += 4) {
    const uint8_t* rb = bits + (int64_t)row * ldb;
    const uint4* r = (const uint4*)rb;
    const uint4* m = (const uint4*)lmask;
    int c = 0, sz = 0;
    unsigned long long h = 0ull;
    // (four 16-byte loads per lane in flight before their first use)
    for (int i0 = lane; i0 < kb16; i0 += 4 * 64) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = i0 + u * 64 < kb16 ? r[i0 + u * 64] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * 64;
        if (i >= kb16) break;
        if (stage) ((uint4*)wrow)[i] = v[u];
        if (use_mask) {
          const uint4 k = m[i];
          c += __builtin_popcount(v[u].x & k.x) + __builtin_popcount(v[u].y & k.y) + __builtin_popcount(v[u].z & k.z) +
               __builtin_popcount(v[u].w & k.w);
        }
        sz += __builtin_popcount(v[u].x) + __builtin_popcount(v[u].y) + __builtin_popcount(v[u].z) +
              __builtin_popcount(v[u].w);
        const unsigned long long w0 = (unsigned long long)v[u].x | ((unsigned long long)v[u].y << 32);
        const unsigned long long w1 = (unsigned long long)v[u].z | ((unsigned long long)v[u].w << 32);
        h += ss_mix(w0 + (unsigned long long)(2 * i + 1) * kSsGolden) +
             ss_mix(w1 + (unsigned long long)(2 * i + 2) * kSsGolden);
      }
    }
    const uint8_t* lb = stage ? wrow : rb;
    if (stage) {  // (this wave's row writes, visible to its own lanes' reads below)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
    for (int j = lane; j < ng; j += 64) {
      const int g = use_mask ? glist[j] : j;
      int any = 0;
      GM2_DBG(goff[g] >= 0 && goff[g] <= goff[g + 1], kDbgMaskPos);
      for (int k = goff[g]; k < goff[g + 1] && !any; ++k) {
        const int p = pos[k];
        GM2_DBG(p >= 0 && p < G, kDbgMaskPos);
        if (p >= 0 && p < G) any = (lb[p >> 3] >> (p & 7)) & 1;
      }
      c += any;
    }
    if (stage) __builtin_amdgcn_wave_barrier();  // (the next row overwrites the buffer after these reads)
    c = ss_wave_sum(c);
    sz = ss_wave_sum(sz);
    h = ss_wave_sum_u64(h);
    if (lane == 0) {
      unsigned long long hash = ss_mix(h + ss_mix((unsigned long long)sz));
      if (hash == kNoKey) hash = kNoKey - 1;
      ckey[row] = c >= min_groups ? ((unsigned long long)sz << 40) | (base + (unsigned long long)row) : kNoKey;
      chash[row] = hash;
      cess[row] = c;
      s_size[row - row0] = sz;
      s_ess[row - row0] = c;
    }
  }
  __syncthreads();
  const int rows = r1 - row0;
  ss_hist_add(s_size, rows, threadIdx.x, (int64_t)G + 1, size_hist);
  ss_hist_add(s_ess, rows, threadIdx.x, (int64_t)ngroups + 1, ess_hist);
  if (wave == 0) {  // (rows <= 64: one wave sees them all)
    const int viable = __popcll(__ballot(lane < rows && s_ess[lane] >= min_groups));
    if (lane == 0) {
      atomicAdd(&totals[0], (unsigned long long)rows);
      if (viable) atomicAdd(&totals[1], (unsigned long long)viable);
    }
  }
}

// the chunk side of a merge: another state's winners (their own keys) as candidates K .. K + n_other
__global__ __launch_bounds__(256) void k_search_take(const unsigned long long* __restrict__ okeys,
                                                   const unsigned long long* __restrict__ ohash,
                                                   const int32_t* __restrict__ oess, const int32_t* __restrict__ ocount,
                                                   int n, unsigned long long* __restrict__ ckey,
                                                   unsigned long long* __restrict__ chash, int32_t* __restrict__ cess) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const bool held = i < *ocount;
  ckey[i] = held ? okeys[i] : kNoKey;
  chash[i] = held ? ohash[i] : 0ull;
  cess[i] = held ? oess[i] : 0;
}

// dst[i] += src[i] (the totals and histograms of a merged state; stream-ordered, one writer)
__global__ __launch_bounds__(256) void k_search_add_i64(const int64_t* __restrict__ src, int64_t n, int64_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] += src[i];
}
__global__ void k_search_or_flag(const int32_t* __restrict__ src, int32_t* __restrict__ dst) {
  if (*src) *dst = *src;
}

// candidate c < K: the old state's winner c (all ones beyond its count); c >= K: chunk row c - K. Every
// eligible candidate claims the slot of its hash (CAS on the empty value, linear probing, at most `slots`
// probes) and lowers the slot's key to its own; the slot is remembered for k_search_mark.
__global__ __launch_bounds__(256) void k_search_insert(const unsigned long long* __restrict__ skeys,
                                                     const unsigned long long* __restrict__ shash,
                                                     const int32_t* __restrict__ scount, int K, int m,
                                                     unsigned long long* __restrict__ cand,
                                                     const unsigned long long* __restrict__ chash,
                                                     unsigned long long* __restrict__ tkey,
                                                     unsigned long long* __restrict__ tmin, unsigned slots,
                                                     int32_t* __restrict__ slotpos, int32_t* __restrict__ error) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  unsigned long long key, h;
  if (c < K) {
    key = c < *scount ? skeys[c] : kNoKey;
    h = c < *scount ? shash[c] : 0ull;
    cand[c] = key;
  } else {
    key = cand[c];
    h = chash[c - K];
  }
  int found = -1;
  if (key != kNoKey) {
    unsigned slot = (unsigned)h & (slots - 1);
    for (unsigned probe = 0; probe < slots; ++probe) {
      GM2_DBG(slot < slots, kDbgMaskPos);
      const unsigned long long prev = atomicCAS(&tkey[slot], kNoKey, h);
      if (prev == kNoKey || prev == h) {
        atomicMin(&tmin[slot], key);
        found = (int)slot;
        break;
      }
      slot = (slot + 1) & (slots - 1);
    }
    if (found < 0) {  // (a full table: cannot happen with slots >= 2 m; the host raises)
      atomicOr(error, 1);
      cand[c] = kNoKey;
    }
  }
  slotpos[c] = found;
}

// a candidate stays eligible when the minimum of its slot is its own key (keys are unique)
__global__ __launch_bounds__(256) void k_search_mark(unsigned long long* __restrict__ cand, int m,
                                                   const unsigned long long* __restrict__ tmin, unsigned slots,
                                                   const int32_t* __restrict__ slotpos) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= m) return;
  const unsigned long long key = cand[c];
  if (key == kNoKey) return;
  const int slot = slotpos[c];
  GM2_DBG(slot >= 0 && (unsigned)slot < slots, kDbgMaskPos);
  if (slot < 0 || (unsigned)slot >= slots || tmin[slot] != key) cand[c] = kNoKey;
}

// One workgroup: the min(K, eligible) smallest of the m candidate keys -> their positions in sel, their
// number in count_out. With more than K eligible keys the K-th smallest is found digit by digit from the
// top: a histogram of the digit over the keys that match the prefix so far, then the bin that holds the
// wanted rank. A lane counts runs of equal digits of its own keys before it touches the LDS bin (the high
// digits of size << 40 | index are nearly constant: one atomic per key would serialise on one bin).
constexpr int kSelThreads = 1024;
__global__ __launch_bounds__(kSelThreads) void k_search_select(const unsigned long long* __restrict__ cand, int m, int K,
                                                             int32_t* __restrict__ sel, int32_t* __restrict__ count_out) {
  __shared__ unsigned hist[256];
  __shared__ unsigned s_count, s_want;
  __shared__ unsigned long long s_prefix;
  const int t = threadIdx.x;
  if (t == 0) s_count = 0u;
  __syncthreads();
  unsigned mine = 0u;
  for (int i = t; i < m; i += kSelThreads) mine += cand[i] != kNoKey;
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  const unsigned eligible = s_count;
  [[maybe_unused]] const unsigned keep = min((unsigned)K, eligible);
  unsigned long long thr = kNoKey - 1;  // (every eligible key)
  if (eligible > (unsigned)K) {          // (uniform over the workgroup)
    if (t == 0) s_want = (unsigned)K, s_prefix = 0ull;
    unsigned long long mask = 0ull;
    for (int shift = 56; shift >= 0; shift -= 8) {
      if (t < 256) hist[t] = 0u;
      __syncthreads();
      const unsigned long long prefix = s_prefix;
      int digit = -1;
      unsigned run = 0u;
      for (int i = t; i < m; i += kSelThreads) {
        const unsigned long long k = cand[i];
        if (k == kNoKey || (k & mask) != prefix) continue;
        const int d = (int)((k >> shift) & 255ull);
        if (d != digit) {
          if (run) atomicAdd(&hist[digit], run);
          digit = d, run = 0u;
        }
        ++run;
      }
      if (run) atomicAdd(&hist[digit], run);
      __syncthreads();
      if (t == 0) {  // the bin of rank s_want (1-based) among the matching keys
        unsigned want = s_want, below = 0u;
        int b = 0;
        while (b < 255 && below + hist[b] < want) below += hist[b++];
        s_want = want - below;
        s_prefix = prefix | ((unsigned long long)b << shift);
      }
      mask |= 255ull << shift;
      __syncthreads();
    }
    thr = s_prefix;
  }
  __syncthreads();
  if (t == 0) s_count = 0u;
  __syncthreads();
  for (int i = t; i < m; i += kSelThreads) {
    const unsigned long long k = cand[i];
    if (k == kNoKey || k > thr) continue;
    const unsigned p = atomicAdd(&s_count, 1u);
    GM2_DBG(p < (unsigned)K, kDbgMaskPos);
    if (p < (unsigned)K) sel[p] = i;
  }
  __syncthreads();
  if (t == 0) {
    GM2_DBG(s_count == keep, kDbgMaskPos);
    *count_out = (int32_t)min(s_count, (unsigned)K);
  }
}

struct SearchSide {  // where a winner comes from / goes to
  const unsigned long long* keys;
  const unsigned long long* hashes;
  const int32_t* essential;
  const uint8_t* rows;
  int64_t ld_rows;
  const float* z;
  int64_t ldz;
};

// one wave per winner j < count: its source position sel[j] < K is the old state's entry, else chunk row
// sel[j] - K (whose key is the candidate key: a winner's was never overwritten)
__global__ __launch_bounds__(256) void k_search_gather(const int32_t* __restrict__ sel, const int32_t* __restrict__ count,
                                                     int K, int m, int kb16, int L, SearchSide st, SearchSide ch,
                                                     const unsigned long long* __restrict__ cand,
                                                     unsigned long long* __restrict__ okeys,
                                                     unsigned long long* __restrict__ ohash, int32_t* __restrict__ oess,
                                                     uint8_t* __restrict__ orows, int64_t old_rows, float* __restrict__ oz,
                                                     int64_t oldz) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= K || j >= *count) return;
  const int src = sel[j];
  GM2_DBG(src >= 0 && src < m, kDbgMaskPos);
  if (src < 0 || src >= m) return;
  const bool old = src < K;
  const int e = old ? src : src - K;
  const SearchSide& s = old ? st : ch;
  if (lane == 0) {
    okeys[j] = old ? s.keys[e] : cand[src];
    ohash[j] = s.hashes[e];
    oess[j] = s.essential[e];
  }
  const uint4* from = (const uint4*)(s.rows + (int64_t)e * s.ld_rows);
  uint4* to = (uint4*)(orows + (int64_t)j * old_rows);
  for (int i = lane; i < kb16; i += 64) to[i] = from[i];
  if (oz) {
    const float* zf = s.z + (int64_t)e * s.ldz;
    float* zt = oz + (int64_t)j * oldz;
    for (int i = lane; i < L; i += 64) zt[i] = zf[i];
  }
}

int64_t up256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// the scratch of one push of n rows into K entries (each array 256-B aligned)
struct SearchScratch {
  int64_t cand, slotpos, chash, cess, sel, table, total;
  unsigned slots;
  SearchScratch(int64_t n, int64_t K) {
    const int64_t m = K + n;
    int64_t t = 16;
    while (t < 2 * m) t <<= 1;
    slots = (unsigned)t;
    int64_t o = 0;
    cand = o, o += up256(8 * m);
    slotpos = o, o += up256(4 * m);
    chash = o, o += up256(8 * std::max<int64_t>(n, 1));
    cess = o, o += up256(4 * std::max<int64_t>(n, 1));
    sel = o, o += up256(4 * K);
    table = o, o += 16 * t;  // [slots] hashes, then [slots] minimum keys
    total = o;
  }
};

// insert, mark, select, gather over the m = K + n candidates whose chunk side is already in scratch
void search_fold(const gm2_search_state& in, const gm2_search_state& out, uint8_t* scratch, const SearchScratch& lo,
                 int64_t n, int64_t G, const SearchSide& chunk, hipStream_t s) {
  const int K = (int)in.K, m = (int)(in.K + n), kb16 = (int)((G + 127) / 128);
  unsigned long long* cand = (unsigned long long*)(scratch + lo.cand);
  unsigned long long* tkey = (unsigned long long*)(scratch + lo.table);
  unsigned long long* tmin = tkey + lo.slots;
  int32_t* slotpos = (int32_t*)(scratch + lo.slotpos);
  int32_t* sel = (int32_t*)(scratch + lo.sel);
  const unsigned grid = (unsigned)((m + 255) / 256);
  {
    TimedLaunch tl(kKcSearchDedupe, s);
    hipLaunchKernelGGL(k_search_insert, dim3(grid), dim3(256), 0, s, (const unsigned long long*)in.keys,
                       (const unsigned long long*)in.hashes, (const int32_t*)in.count, K, m, cand,
                       (const unsigned long long*)(scratch + lo.chash), tkey, tmin, lo.slots, slotpos, out.error);
    GM2_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_search_mark, dim3(grid), dim3(256), 0, s, cand, m, (const unsigned long long*)tmin, lo.slots,
                       (const int32_t*)slotpos);
    GM2_CHECK_LAUNCH();
  }
  {
    TimedLaunch tl(kKcSearchSelect, s);
    hipLaunchKernelGGL(k_search_select, dim3(1), dim3(kSelThreads), 0, s, (const unsigned long long*)cand, m, K, sel,
                       out.count);
    GM2_CHECK_LAUNCH();
  }
  TimedLaunch tl(kKcSearchGather, s);
  SearchSide st{(const unsigned long long*)in.keys, (const unsigned long long*)in.hashes, in.essential, in.rows,
                in.ld_rows, in.z, in.ldz};
  hipLaunchKernelGGL(k_search_gather, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, s, (const int32_t*)sel,
                     (const int32_t*)out.count, K, m, kb16, (int)in.L, st, chunk, (const unsigned long long*)cand,
                     (unsigned long long*)out.keys, (unsigned long long*)out.hashes, out.essential, out.rows, out.ld_rows,
                     out.z, out.ldz);
  GM2_CHECK_LAUNCH();
}

void clear_table(uint8_t* scratch, const SearchScratch& lo, hipStream_t s) {
  if (hipMemsetAsync(scratch + lo.table, 0xff, (size_t)16 * lo.slots, s) != hipSuccess) throw Gm2Error("hipMemsetAsync");
}

}  // namespace

size_t search_scratch_bytes(int64_t n_max, int64_t K) { return (size_t)SearchScratch(n_max, K).total; }

void launch_search_push(const gm2_search_state& in, const gm2_search_state& out, void* scratch, const uint8_t* bits,
                        int64_t n, int64_t ldb, int64_t G, const float* z, int64_t ldz, int64_t base,
                        const int32_t* goff, int64_t ngroups, const int32_t* pos, int64_t min_groups, hipStream_t s) {
  if (n <= 0) return;
  const SearchScratch lo(n, in.K);
  uint8_t* sc = (uint8_t*)scratch;
  {
    TimedLaunch tl(kKcSearchDedupe, s);
    clear_table(sc, lo, s);
  }
  // (the group mask + list in LDS when they fit 60 KB -- the kernel's own arrays take the rest of the 64 KB
  // of a workgroup --, each wave's row buffer too when that still fits)
  const int64_t kb = (G + 127) / 128 * 16;
  const int64_t lds_mask = ((kb + ngroups * 4 + 15) & ~(int64_t)15);
  const int use_mask = ngroups > 0 && lds_mask <= 60 * 1024;
  const int stage = use_mask && lds_mask + 4 * kb <= 60 * 1024;
  const int64_t lds = use_mask ? (stage ? lds_mask + 4 * kb : lds_mask) : 0;
  unsigned long long* cand = (unsigned long long*)(sc + lo.cand);
  {
    TimedLaunch tl(kKcSearchScore, s);
    hipLaunchKernelGGL(k_search_score, dim3((unsigned)((n + kSsRows - 1) / kSsRows)), dim3(256), (unsigned)lds, s, bits,
                       (int)n, ldb, (int)(kb / 16), (int)G, goff, (int)ngroups, pos, (int)std::min<int64_t>(min_groups, 0x7fffffff),
                       (unsigned long long)base, cand + in.K, (unsigned long long*)(sc + lo.chash), (int32_t*)(sc + lo.cess),
                       (unsigned long long*)out.totals, (unsigned long long*)out.size_hist,
                       (unsigned long long*)out.ess_hist, use_mask, stage);
    GM2_CHECK_LAUNCH();
  }
  SearchSide chunk{nullptr, (const unsigned long long*)(sc + lo.chash), (const int32_t*)(sc + lo.cess), bits, ldb, z, ldz};
  search_fold(in, out, sc, lo, n, G, chunk, s);
}

void launch_search_merge(const gm2_search_state& in, const gm2_search_state& out, void* scratch,
                         const gm2_search_state& other, int64_t G, int64_t ngroups, hipStream_t s) {
  const int64_t n = other.K;
  const SearchScratch lo(n, in.K);
  uint8_t* sc = (uint8_t*)scratch;
  clear_table(sc, lo, s);
  unsigned long long* cand = (unsigned long long*)(sc + lo.cand);
  hipLaunchKernelGGL(k_search_take, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s,
                     (const unsigned long long*)other.keys, (const unsigned long long*)other.hashes,
                     (const int32_t*)other.essential, (const int32_t*)other.count, (int)n, cand + in.K,
                     (unsigned long long*)(sc + lo.chash), (int32_t*)(sc + lo.cess));
  GM2_CHECK_LAUNCH();
  auto add = [&](const int64_t* src, int64_t cnt, int64_t* dst) {
    hipLaunchKernelGGL(k_search_add_i64, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, src, cnt, dst);
    GM2_CHECK_LAUNCH();
  };
  add(other.totals, 2, out.totals);
  add(other.size_hist, G + 1, out.size_hist);
  add(other.ess_hist, ngroups + 1, out.ess_hist);
  hipLaunchKernelGGL(k_search_or_flag, dim3(1), dim3(1), 0, s, (const int32_t*)other.error, out.error);
  GM2_CHECK_LAUNCH();
  SearchSide chunk{nullptr, (const unsigned long long*)(sc + lo.chash), (const int32_t*)(sc + lo.cess), other.rows,
                   other.ld_rows, other.z, other.ldz};
  search_fold(in, out, sc, lo, n, G, chunk, s);
}

#ifdef GM2_DEBUG
GM2_DBG_TAKE_FN(dbg_take_search)
#endif

}  // namespace gm2
