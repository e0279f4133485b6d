// binning.hip — the (tile, splat) pairs every kind renders from, for gfx950: per-tile count -> scan -> bucket -> per-tile
// depth sort; and the deterministic rows that those pairs number (the 3DGS and 2DGS backward, the mask vote).
//
// The pipeline does not follow the CUDA original's duplicate-with-64-bit-keys + global radix sort: (tile,splat) pairs are
// counted per tile while projecting, bucketed by tile with one atomic per pair, and each tile's list (a few hundred
// entries) is depth-sorted in LDS by the workgroup that owns the tile.  Ties in depth are broken by splat index, which
// makes the order — and therefore the image — independent of atomic arrival order.
#include <stdlib.h>

#include "common.hpp"

namespace scorp {
namespace {

// ---------------------------------------------------------------------------------------------------------
// K2: exclusive prefix sum of the per-tile counts (one workgroup; T is 7.5k at 1600x1200, <100k at 5400x4050).
// ---------------------------------------------------------------------------------------------------------
// The exclusive prefix of `sum` over the workgroup's 1024 threads, and in *total their sum: shuffles inside each wave, the
// 16 wave totals through LDS (s_wave[16]; two barriers instead of the twenty of a Hillis-Steele over LDS)
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t sum, uint32_t *s_wave, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
    if (lane >= off) incl += v;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  if (wave == 0) {
    uint32_t w = lane < 16 ? s_wave[lane] : 0u;
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)w, off, 64);
      if (lane >= off) w += v;
    }
    if (lane < 16) s_wave[lane] = w;   // inclusive totals of waves 0..lane
  }
  __syncthreads();
  incl += wave > 0 ? s_wave[wave - 1] : 0u;
  *total = s_wave[15];
  return incl - sum;
}

__global__ void __launch_bounds__(1024)
scan_tiles_kernel(const uint32_t *__restrict__ tile_count, uint32_t *__restrict__ tile_start, int tiles,
                  StateHeader *__restrict__ header) {
  __shared__ uint32_t s_wave[16];
  const int t = threadIdx.x;
  const int per = (tiles + 1023) / 1024;
  const int lo = min(tiles, t * per), hi = min(tiles, lo + per);
  // the thread's counts stay in registers between the two passes when they fit (per <= 8: up to 8192 tiles)
  uint32_t cnt[8];
  uint32_t sum = 0;
  if (per <= 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) cnt[j] = lo + j < hi ? tile_count[lo + j] : 0u;
#pragma unroll
    for (int j = 0; j < 8; j++) sum += cnt[j];
  } else {
    for (int k = lo; k < hi; k++) sum += tile_count[k];
  }
  uint32_t total;
  uint32_t run = block_scan_1024(sum, s_wave, &total);
  uint2 *range = reinterpret_cast<uint2 *>(tile_start);   // (start, end) per tile
  if (per <= 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (lo + j < hi) range[lo + j] = make_uint2(run, run + cnt[j]);
      run += cnt[j];
    }
  } else {
    for (int k = lo; k < hi; k++) {
      const uint32_t c = tile_count[k];
      range[k] = make_uint2(run, run + c);
      run += c;
    }
  }
  if (t == 1023) {
    header->num_pairs = total;
    header->overflow = 0;
  }
}

// The same scan for up to kMaxLdsTiles tiles with the counts staged in LDS: coalesced, independent loads and stores (the
// kernel above walks `per` consecutive counts per thread with dependent, uncoalesced global loads - 56 us for the 37 500
// tiles of the align sweep's 15 stacked views, all of it latency).
__global__ void __launch_bounds__(1024)
scan_tiles_lds_kernel(const uint32_t *__restrict__ tile_count, uint32_t *__restrict__ tile_start, int tiles,
                      StateHeader *__restrict__ header) {
  extern __shared__ uint32_t s_all[];
  __shared__ uint32_t s_wave[16];
  const int t = threadIdx.x;
  for (int k = t; k < tiles; k += 1024) s_all[k] = tile_count[k];
  __syncthreads();
  const int per = (tiles + 1023) / 1024;
  const int lo = min(tiles, t * per), hi = min(tiles, lo + per);
  uint32_t sum = 0;
  for (int k = lo; k < hi; k++) sum += s_all[k];
  uint32_t total;
  uint32_t run = block_scan_1024(sum, s_wave, &total);
  uint2 *range = reinterpret_cast<uint2 *>(tile_start);   // (start, end) per tile
  for (int k = lo; k < hi; k++) {
    const uint32_t v = s_all[k];
    range[k] = make_uint2(run, run + v);
    run += v;
  }
  if (t == 0) {
    header->num_pairs = total;
    header->overflow = 0;
  }
}

// ---------------------------------------------------------------------------------------------------------
// K3: bucket (tile,splat) pairs by tile. The per-tile counter doubles as the cursor (counted back down to zero,
// so it is clean for the next view). Slot order inside a tile is arbitrary; the sort below fixes it.
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
scatter_pairs_kernel(int N, const BinRec *__restrict__ bin, const uint64_t *__restrict__ tile_mask,
                     uint32_t *__restrict__ tile_count,
                     const uint32_t *__restrict__ tile_start, int tiles_x, uint64_t *__restrict__ keys,
                     uint32_t capacity, StateHeader *__restrict__ header, uint32_t *__restrict__ header_copy) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) {
    header->capacity = capacity;
    header->long_tiles = 0;   // (the sort's list of long tiles starts empty)
    const uint32_t np = header->num_pairs, ov = np > capacity ? 1u : header->overflow;
    if (np > capacity) header->overflow = 1;
    if (header_copy) { header_copy[0] = np; header_copy[1] = ov; header_copy[2] = capacity; header_copy[3] = 0u; }
  }
  if (i >= N) return;
  const uint4 raw = reinterpret_cast<const uint4 *>(bin)[i];
  const BinRec br = *reinterpret_cast<const BinRec *>(&raw);
  if ((br.radius & kRadiusMask) == 0) return;
  const uint64_t key = ((uint64_t)br.depth_bits << 32) | (uint32_t)i;
  for_each_tile(br.x0, br.y0, br.x1, br.y1, tile_mask[i], tiles_x, [&](int t) {
    const uint32_t slot = tile_start[2 * t] + atomicSub(&tile_count[t], 1u) - 1u;
    if (slot < capacity) keys[slot] = key;
  });
}

// ---------------------------------------------------------------------------------------------------------
// LDS-histogram binning (the default).  Device-scope atomics on random addresses execute at the memory side, one
// request per lane (~14 G/s measured here), so counting and bucketing 3.3 M pairs through global counters cost
// ~450 us.  Instead each block owns a contiguous range of Gaussians and a private per-tile histogram in LDS:
//   count : LDS atomics; the histogram is written out as one coalesced row  hist[block][tile];
//   scan  : per tile, an exclusive prefix over blocks (column of hist, coalesced across threads) + the tile total;
//           then the existing single-block scan of the totals gives tile_start;
//   scatter: the block reloads its row (+ tile_start) as LDS cursors and ranks its pairs with returning LDS atomics.
// Slot order inside a tile is arbitrary but deterministic; the per-tile depth sort fixes the final order.
// ---------------------------------------------------------------------------------------------------------
constexpr int kBinAhead = 4;         // Gaussians whose records one thread loads together
constexpr int kBinThreads = 1024;   // few Gaussians per thread: the count / scatter loops are latency chains (load -> LDS atomic -> store)

// Images with more tiles than one LDS histogram holds are binned in passes: workgroup (pass, block) owns the tile range
// [pass * tpp, (pass + 1) * tpp) of bin block `block` (blockIdx.x = pass * nb + block).
// kCells: the bins are cells of kCellTiles x kCellTiles tiles (`tiles` = number of cells, `tiles_x` = cells per row): the
// first level of the two-level binning
template <bool kCells>
__global__ void __launch_bounds__(kBinThreads)
count_tiles_lds_kernel(int N, int per_block, int nb, int tpp, int view_n, const BinRec *__restrict__ bin,
                       const uint64_t *__restrict__ tile_mask, int tiles, int tiles_x, uint32_t *__restrict__ block_hist,
                       StateHeader *__restrict__ header) {
  extern __shared__ uint32_t s_hist[];
  if (header && blockIdx.x == 0 && threadIdx.x == 0) { header->num_pairs = 0; header->overflow = 0; }   // scan_block_hist adds the totals up
  const int pass = blockIdx.x / nb, blk = blockIdx.x - pass * nb;
  const int t_lo = pass * tpp, nt = min(tiles - t_lo, tpp);
  for (int t = threadIdx.x; t < nt; t += kBinThreads) s_hist[t] = 0;
  __syncthreads();
  // (stacked views: pass v looks at view v's Gaussians only, [v * view_n, (v + 1) * view_n))
  const int g0 = view_n >= 0 ? pass * view_n : 0, g1 = view_n >= 0 ? g0 + view_n : N;
  const int lo = g0 + blk * per_block, hi = min(g1, lo + per_block);
  // (the loads of kBinAhead Gaussians are issued together: one thread walks 2 - 4 of them, and with a load per iteration that
  // was as many dependent round trips to memory)
  for (int i0 = lo + threadIdx.x; i0 < hi; i0 += kBinAhead * kBinThreads) {
    uint4 raws[kBinAhead];
    uint64_t masks[kBinAhead];
#pragma unroll
    for (int u = 0; u < kBinAhead; u++) {
      const int i = min(i0 + u * kBinThreads, hi - 1);
      raws[u] = reinterpret_cast<const uint4 *>(bin)[i];
      masks[u] = tile_mask[i];
    }
#pragma unroll
    for (int u = 0; u < kBinAhead; u++) {
      if (i0 + u * kBinThreads >= hi) break;
      const BinRec br = *reinterpret_cast<const BinRec *>(&raws[u]);
      const uint64_t mask = masks[u];
      if ((br.radius & kRadiusMask) == 0) continue;
      if constexpr (kCells) {
        for_each_tile_xy(br.x0, br.y0, br.x1, br.y1, mask, [&](int x, int y) {
          atomicAdd(&s_hist[(y / kCellTiles) * tiles_x + x / kCellTiles], 1u);
        });
      } else {
        for_each_tile(br.x0, br.y0, br.x1, br.y1, mask, tiles_x, [&](int t) {
          const uint32_t r = (uint32_t)(t - t_lo);
          if (r < (uint32_t)nt) atomicAdd(&s_hist[r], 1u);
        });
      }
    }
  }
  __syncthreads();
  uint32_t *row = block_hist + (size_t)blk * tiles + t_lo;
  for (int t = threadIdx.x; t < nt; t += kBinThreads) row[t] = s_hist[t];
}

// 32 tiles x 32 segments of the block range per workgroup (235 workgroups at 7500 tiles — enough to cover every CU;
// the first form, 64 x 16, left half the chip idle): each thread sums its blocks for one tile (coalesced 128-byte
// rows), the segment totals are exchanged through LDS, then the prefixes are written in place.
constexpr int kScanTiles = 32, kScanSegs = 32;
__global__ void __launch_bounds__(kScanTiles * kScanSegs)
scan_block_hist_kernel(int nb, int tiles, uint32_t *__restrict__ block_hist, uint32_t *__restrict__ tile_count,
                       StateHeader *__restrict__ header) {
  __shared__ uint32_t s_seg[kScanSegs][kScanTiles];
  const int tl = threadIdx.x % kScanTiles, seg = threadIdx.x / kScanTiles;
  const int t = blockIdx.x * kScanTiles + tl;
  const int per = (nb + kScanSegs - 1) / kScanSegs;
  const int b0 = min(nb, seg * per), b1 = min(nb, b0 + per);
  // the segment's counts stay in registers between the two passes (nb <= 512 -> at most 16 per thread), and all of
  // its loads are in flight together instead of one per loop iteration
  constexpr int kMaxPer = (kBinBlocksMax + kScanSegs - 1) / kScanSegs;
  uint32_t cnt[kMaxPer];
  uint32_t sum = 0;
#pragma unroll
  for (int j = 0; j < kMaxPer; j++) {
    const int b = b0 + j;
    cnt[j] = (t < tiles && b < b1) ? block_hist[(size_t)b * tiles + t] : 0u;
  }
#pragma unroll
  for (int j = 0; j < kMaxPer; j++) sum += cnt[j];
  s_seg[seg][tl] = sum;
  __syncthreads();
  uint32_t run = 0;
  for (int q = 0; q < seg; q++) run += s_seg[q][tl];
  if (t < tiles) {
#pragma unroll
    for (int j = 0; j < kMaxPer; j++) {
      const int b = b0 + j;
      if (b < b1) block_hist[(size_t)b * tiles + t] = run;
      run += cnt[j];
    }
    if (seg == kScanSegs - 1) tile_count[t] = run;
  }
  if (header && seg == kScanSegs - 1) {   // D = the sum of the tile totals: this workgroup's 32 (lanes 32..63 of its last wave)
    static_assert(kScanTiles == 32, "the last segment is the upper half of a wave");
    uint32_t tot = t < tiles ? run : 0u;
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) tot += (uint32_t)__shfl_xor((int)tot, off, 64);
    if (tl == 0 && tot) atomicAdd(&header->num_pairs, tot);
  }
}

// kCells: bins are cells (see count_tiles_lds_kernel); `tile_start` is then the plain prefix cell_start[cells + 1] and a key
// carries its tile's index inside the cell in bits kCellShift.. of its low word (expand_cells_kernel strips it again)
template <bool kCells>
__global__ void __launch_bounds__(kBinThreads)
scatter_pairs_lds_kernel(int N, int per_block, int nb, int tpp, int view_n, const BinRec *__restrict__ bin,
                         const uint64_t *__restrict__ tile_mask, int tiles, int tiles_x,
                         const uint32_t *__restrict__ block_hist, uint32_t *__restrict__ tile_start,
                         const uint32_t *__restrict__ tile_count, uint64_t *__restrict__ keys, uint32_t capacity,
                         StateHeader *__restrict__ header, uint32_t *__restrict__ header_copy) {
  extern __shared__ uint32_t s_cur[];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    header->capacity = capacity;
    header->long_tiles = 0;   // (the sort's list of long tiles starts empty)
    const uint32_t np = header->num_pairs, ov = np > capacity ? 1u : header->overflow;
    if (np > capacity) header->overflow = 1;
    if (header_copy) { header_copy[0] = np; header_copy[1] = ov; header_copy[2] = capacity; header_copy[3] = 0u; }
  }
  const int pass = blockIdx.x / nb, blk = blockIdx.x - pass * nb;
  const int t_lo = pass * tpp, nt = min(tiles - t_lo, tpp);
  const uint32_t *row = block_hist + (size_t)blk * tiles + t_lo;
  if (tile_count) {
    // (one pass, tiles <= 8192) tile_start is not there yet: every workgroup takes the exclusive prefix of the tile
    // totals itself - 8 counts per thread, wave scans, the 16 wave totals through LDS - straight into its cursors;
    // workgroup 0 also writes it out for the sort and the blend kernels
    static_assert(kBinThreads == 1024, "8 counts per thread cover 8192 tiles");
    __shared__ uint32_t s_wave[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t cnt[8], rw[8], sum = 0;
    if ((tiles & 3) == 0 && 8 * t + 8 <= tiles) {   // rows of the histogram matrix are 16-byte aligned when tiles % 4 == 0
      const uint4 c0 = reinterpret_cast<const uint4 *>(tile_count)[2 * t], c1 = reinterpret_cast<const uint4 *>(tile_count)[2 * t + 1];
      const uint4 r0 = reinterpret_cast<const uint4 *>(row)[2 * t], r1 = reinterpret_cast<const uint4 *>(row)[2 * t + 1];
      cnt[0] = c0.x; cnt[1] = c0.y; cnt[2] = c0.z; cnt[3] = c0.w; cnt[4] = c1.x; cnt[5] = c1.y; cnt[6] = c1.z; cnt[7] = c1.w;
      rw[0] = r0.x; rw[1] = r0.y; rw[2] = r0.z; rw[3] = r0.w; rw[4] = r1.x; rw[5] = r1.y; rw[6] = r1.z; rw[7] = r1.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const bool in = 8 * t + j < tiles;
        cnt[j] = in ? tile_count[8 * t + j] : 0u;
        rw[j] = in ? row[8 * t + j] : 0u;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) sum += cnt[j];
    uint32_t incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t v = (uint32_t)__shfl_up((int)incl, off, 64);
      if (lane >= off) incl += v;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (int w = 0; w < wave; w++) run += s_wave[w];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (8 * t + j < tiles) {
        s_cur[8 * t + j] = run + rw[j];
        if (blockIdx.x == 0) {
          if constexpr (kCells) tile_start[8 * t + j] = run;
          else reinterpret_cast<uint2 *>(tile_start)[8 * t + j] = make_uint2(run, run + cnt[j]);
        }
      }
      run += cnt[j];
    }
    if (kCells && blockIdx.x == 0 && t == kBinThreads - 1) tile_start[tiles] = run;
  } else {
    for (int t = threadIdx.x; t < nt; t += kBinThreads) s_cur[t] = tile_start[2 * (t_lo + t)] + row[t];
  }
  __syncthreads();
  const int g0 = view_n >= 0 ? pass * view_n : 0, g1 = view_n >= 0 ? g0 + view_n : N;
  const int lo = g0 + blk * per_block, hi = min(g1, lo + per_block);
  for (int i0 = lo + threadIdx.x; i0 < hi; i0 += kBinAhead * kBinThreads) {
    uint4 raws[kBinAhead];
    uint64_t masks[kBinAhead];
#pragma unroll
    for (int u = 0; u < kBinAhead; u++) {
      const int i = min(i0 + u * kBinThreads, hi - 1);
      raws[u] = reinterpret_cast<const uint4 *>(bin)[i];
      masks[u] = tile_mask[i];
    }
#pragma unroll
    for (int u = 0; u < kBinAhead; u++) {
    const int i = i0 + u * kBinThreads;
    if (i >= hi) break;
    const BinRec br = *reinterpret_cast<const BinRec *>(&raws[u]);
    const uint64_t mask = masks[u];
    if ((br.radius & kRadiusMask) == 0) continue;
    const uint64_t key = ((uint64_t)br.depth_bits << 32) | (uint32_t)i;
    if constexpr (kCells) {
      for_each_tile_xy(br.x0, br.y0, br.x1, br.y1, mask, [&](int x, int y) {
        const uint32_t slot = atomicAdd(&s_cur[(y / kCellTiles) * tiles_x + x / kCellTiles], 1u);
        if (slot < capacity) keys[slot] = key | (uint64_t)((uint32_t)((y % kCellTiles) * kCellTiles + x % kCellTiles) << kCellShift);
      });
    } else {
      for_each_tile(br.x0, br.y0, br.x1, br.y1, mask, tiles_x, [&](int t) {
        const uint32_t r = (uint32_t)(t - t_lo);
        if (r < (uint32_t)nt) {
          const uint32_t slot = atomicAdd(&s_cur[r], 1u);
          if (slot < capacity) keys[slot] = key;
        }
      });
    }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Second level of the two-level binning: ONE WORKGROUP PER CELL.  The cell's keys (contiguous, in arbitrary order) are
// counted per tile (sixteen LDS counters), the sixteen tile buckets are laid out one after the other inside the cell's own
// range of the second key buffer, every tile's (start, end) is written, and the keys go to their buckets with the tile
// index stripped - so that what the per-tile sort reads is exactly what the one-level scatter produces.  Up to
// kExpandKeep keys per thread stay in registers between the two passes (a cell of S3 holds ~5 100 pairs); longer cells read
// the rest again.  A view that overflowed its reservation is clamped to `capacity` as everywhere else.
// (Staging the buckets in LDS and copying them out linearly - a wave's 64 stores consecutive instead of scattered over the
// cell's 40 KB - was built and is SLOWER, 19.1 against 16.2 us: with 64 KB of LDS two workgroups share a CU, and the kernel
// is a chain of round trips, not a stream of stores.)
// ---------------------------------------------------------------------------------------------------------
constexpr int kExpandThreads = 512, kExpandKeep = 12;
__global__ void __launch_bounds__(kExpandThreads)
expand_cells_kernel(const uint32_t *__restrict__ cell_start, const uint64_t *__restrict__ keys_in, uint64_t *__restrict__ keys_out,
                    uint32_t *__restrict__ tile_range, uint32_t capacity, int cells_x, int tiles_x, int tiles_y) {
  constexpr int kBins = kCellTiles * kCellTiles;
  __shared__ uint32_t s_cnt[kBins], s_cur[kBins];
  const int cell = blockIdx.x, tid = threadIdx.x;
  const uint32_t beg = min(cell_start[cell], capacity), end = min(cell_start[cell + 1], capacity);
  if (tid < kBins) s_cnt[tid] = 0;
  __syncthreads();
  uint64_t kk[kExpandKeep];
#pragma unroll
  for (int j = 0; j < kExpandKeep; j++) {
    const uint32_t i = beg + tid + j * kExpandThreads;
    kk[j] = i < end ? keys_in[i] : ~0ull;
  }
  auto bin_of = [](uint64_t k) { return (uint32_t)(k >> kCellShift) & (uint32_t)(kBins - 1); };
#pragma unroll
  for (int j = 0; j < kExpandKeep; j++)
    if (beg + tid + j * kExpandThreads < end) atomicAdd(&s_cnt[bin_of(kk[j])], 1u);
  for (uint32_t i = beg + tid + kExpandKeep * kExpandThreads; i < end; i += kExpandThreads) atomicAdd(&s_cnt[bin_of(keys_in[i])], 1u);
  __syncthreads();
  if (tid < kBins) {
    uint32_t run = beg;
    for (int b = 0; b < tid; b++) run += s_cnt[b];
    s_cur[tid] = run;
    const int tx = (cell % cells_x) * kCellTiles + tid % kCellTiles, ty = (cell / cells_x) * kCellTiles + tid / kCellTiles;
    if (tx < tiles_x && ty < tiles_y) reinterpret_cast<uint2 *>(tile_range)[ty * tiles_x + tx] = make_uint2(run, run + s_cnt[tid]);
  }
  __syncthreads();
  constexpr uint64_t kStrip = ~((uint64_t)(kBins - 1) << kCellShift);
#pragma unroll
  for (int j = 0; j < kExpandKeep; j++)
    if (beg + tid + j * kExpandThreads < end) keys_out[atomicAdd(&s_cur[bin_of(kk[j])], 1u)] = kk[j] & kStrip;
  for (uint32_t i = beg + tid + kExpandKeep * kExpandThreads; i < end; i += kExpandThreads) {
    const uint64_t k = keys_in[i];
    keys_out[atomicAdd(&s_cur[bin_of(k)], 1u)] = k & kStrip;
  }
}

// ---------------------------------------------------------------------------------------------------------
// K4: per-tile depth sort. One workgroup per tile; bitonic network (all-ascending "flip" form, so virtual +inf
// padding never moves) in LDS for lists up to kSortLds entries, in global memory (same network) beyond that.
// Output: point_list = splat indices front to back.
// ---------------------------------------------------------------------------------------------------------
constexpr int kSortLds = 4096;  // 32 KiB of 64-bit keys

__device__ __forceinline__ void ce(uint64_t &lo, uint64_t &hi) {   // compare-exchange, ascending
  const uint64_t u = lo, v = hi;
  const bool sw = u > v;
  lo = sw ? v : u; hi = sw ? u : v;
}

// The network on P (a power of two >= n) keys in place at `a`, 256 threads, a workgroup barrier in front of every stage:
// the lists beyond kSortLds entries, in global memory.
__device__ __forceinline__ void bitonic_sort(uint64_t *a, uint32_t n, uint32_t P) {
  const uint32_t tid = threadIdx.x;
  for (uint32_t lk = 1; (1u << lk) <= P; lk++) {
    const uint32_t k = 1u << lk, half = k >> 1;
    __syncthreads();
    for (uint32_t i = tid; i < (P >> 1); i += 256) {  // flip step: lo <-> mirrored partner inside each k-block
      const uint32_t base = (i >> (lk - 1)) << lk, r = i & (half - 1);
      const uint32_t lo = base + r, hi = base + (k - 1 - r);
      if (hi < n) {
        const uint64_t u = a[lo], v = a[hi];
        if (u > v) { a[lo] = v; a[hi] = u; }
      }
    }
    for (int lj = (int)lk - 2; lj >= 0; lj--) {
      const uint32_t j = 1u << lj;
      __syncthreads();
      for (uint32_t i = tid; i < (P >> 1); i += 256) {
        const uint32_t lo = ((i >> lj) << (lj + 1)) + (i & (j - 1));
        const uint32_t hi = lo + j;
        if (hi < n) {
          const uint64_t u = a[lo], v = a[hi];
          if (u > v) { a[lo] = v; a[hi] = u; }
        }
      }
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------
// K4, lists of up to 1024 entries (nearly all of them): the same bitonic network with the keys IN REGISTERS.  Thread t
// owns the four consecutive keys 4t .. 4t+3, a wave 256 consecutive keys.  Every comparator of the network pairs
// element e with e ^ X (X = k - 1 for the flip step of level k, X = j for a half-cleaner), i.e. lane ^ (X / 4) with the
// registers in the same (cleaner) or reversed (flip) order, and the lower index keeps the minimum:
//   * X < 4                : inside a thread;
//   * lane masks 1,2,3,7,8,15: one DPP move per dword (quad_perm / row_half_mirror / row_ror:8 / row_mirror), 4 = 7 o 3;
//   * lane masks 16,31,32,63 : ds_bpermute (the LDS crossbar, no LDS memory);
//   * X >= 256             : between waves, through LDS (2 stages of 45 for 512 keys, 5 of 55 for 1024).
// No LDS round trip and no barrier for all the rest, which the LDS version paid per stage.  Waves whose keys are all
// padding leave at once (the network of size P never touches indices >= P).
// ---------------------------------------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ uint32_t xor_lane32(uint32_t v, int bperm_addr) {
  if constexpr (M == 1) return __builtin_amdgcn_update_dpp(0u, v, 0xB1, 0xF, 0xF, false);        // quad_perm [1,0,3,2]
  else if constexpr (M == 2) return __builtin_amdgcn_update_dpp(0u, v, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
  else if constexpr (M == 3) return __builtin_amdgcn_update_dpp(0u, v, 0x1B, 0xF, 0xF, false);   // quad_perm [3,2,1,0]
  else if constexpr (M == 7) return __builtin_amdgcn_update_dpp(0u, v, 0x141, 0xF, 0xF, false);  // row_half_mirror
  else if constexpr (M == 15) return __builtin_amdgcn_update_dpp(0u, v, 0x140, 0xF, 0xF, false); // row_mirror
  else if constexpr (M == 8) return __builtin_amdgcn_update_dpp(0u, v, 0x128, 0xF, 0xF, false);  // row_ror:8
  else if constexpr (M == 4) return xor_lane32<7>(xor_lane32<3>(v, 0), 0);
  else return (uint32_t)__builtin_amdgcn_ds_bpermute(bperm_addr, (int)v);                          // 16, 31, 32, 63
}
template <int M>
__device__ __forceinline__ uint64_t xor_lane64(uint64_t v, int bperm_addr) {
  const uint32_t lo = xor_lane32<M>((uint32_t)v, bperm_addr), hi = xor_lane32<M>((uint32_t)(v >> 32), bperm_addr);
  return ((uint64_t)hi << 32) | lo;
}
// one network stage between lanes: element (lane, r) against (lane ^ M, FLIP ? 3 - r : r); keep_min per lane
template <int M, bool FLIP>
__device__ __forceinline__ void lane_stage(uint64_t (&k)[4], bool keep_min, int lane) {
  const int addr = ((lane ^ M) & 63) << 2;
  uint64_t p[4];
#pragma unroll
  for (int r = 0; r < 4; r++) p[r] = xor_lane64<M>(k[FLIP ? 3 - r : r], addr);
#pragma unroll
  for (int r = 0; r < 4; r++) k[r] = ((p[r] < k[r]) == keep_min) ? p[r] : k[r];
}
// one network stage between waves, through LDS: element e against e ^ X (X >= 256; FLIP: X = K - 1)
template <bool FLIP>
__device__ __forceinline__ void cross_stage(uint64_t (&k)[4], uint64_t *s_x, uint32_t base, uint32_t X, bool keep_min) {
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  u64x2 *mine = reinterpret_cast<u64x2 *>(s_x + base);
  u64x2 w0, w1;
  w0.x = k[0]; w0.y = k[1]; w1.x = k[2]; w1.y = k[3];
  mine[0] = w0; mine[1] = w1;
  __syncthreads();
  const u64x2 *theirs = reinterpret_cast<const u64x2 *>(s_x + (base ^ (X & ~3u)));
  const u64x2 t0 = theirs[0], t1 = theirs[1];
  const uint64_t q[4] = {t0.x, t0.y, t1.x, t1.y};
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint64_t p = q[FLIP ? 3 - r : r];
    k[r] = ((p < k[r]) == keep_min) ? p : k[r];
  }
  __syncthreads();   // everyone has read before the next cross stage overwrites
}
__device__ __forceinline__ void thread_tail(uint64_t (&k)[4]) {   // j = 2, j = 1 of any level
  ce(k[0], k[2]); ce(k[1], k[3]);
  ce(k[0], k[1]); ce(k[2], k[3]);
}
// level K of the network (flip, half-cleaners down to j = 4, then the in-thread tail), lane masks as template constants
template <int K>
__device__ __forceinline__ void sort_level(uint64_t (&k)[4], uint64_t *s_x, uint32_t base, int lane) {
  constexpr int FM = K / 4 - 1;   // lane mask of the flip
  if constexpr (FM < 64) lane_stage<FM, true>(k, (lane & (K / 8)) == 0, lane);
  else cross_stage<true>(k, s_x, base, (uint32_t)K - 1u, (base & (K / 2)) == 0);
#define SCORP_CLEAN(J)                                                                                   \
  if constexpr (K / 4 >= (J) && (J) >= 4) {                                                              \
    if constexpr ((J) / 4 < 64) lane_stage<((J) / 4 < 64 ? (J) / 4 : 1), false>(k, (lane & ((J) / 4)) == 0, lane); \
    else cross_stage<false>(k, s_x, base, (uint32_t)(J), (base & (J)) == 0);                             \
  }
  SCORP_CLEAN(256) SCORP_CLEAN(128) SCORP_CLEAN(64) SCORP_CLEAN(32) SCORP_CLEAN(16) SCORP_CLEAN(8) SCORP_CLEAN(4)
#undef SCORP_CLEAN
  thread_tail(k);
}

__global__ void __launch_bounds__(256)
sort_tiles_reg_kernel(const uint32_t *__restrict__ tile_start, const uint64_t *__restrict__ keys,
                      uint32_t *__restrict__ point_list, uint32_t capacity, uint32_t *__restrict__ long_list,
                      StateHeader *__restrict__ header) {
  __shared__ __attribute__((aligned(16))) uint64_t s_x[1024];
  const int tile = blockIdx.x;
  const TileRange tr = tile_range(tile_start, tile, capacity);
  const uint32_t beg = tr.beg, n = tr.end - tr.beg;
  if (n > 1024) {   // sort_tiles_long_kernel's: it walks the list of such tiles (usually empty) instead of every tile
    if (threadIdx.x == 0) long_list[atomicAdd(&header->long_tiles, 1u)] = (uint32_t)tile;
    return;
  }
  if (n == 0) return;
  const uint32_t base = 4 * threadIdx.x;
  uint32_t P = 4;
  while (P < n) P <<= 1;
  if (256u * (threadIdx.x >> 6) >= P) return;   // whole waves of padding leave (never single lanes: lanes exchange)
  const int lane = threadIdx.x & 63;
  constexpr uint64_t kInf = ~0ull;
  uint64_t k[4];
#pragma unroll
  for (int r = 0; r < 4; r++) k[r] = base + r < n ? keys[beg + base + r] : kInf;
  ce(k[0], k[1]); ce(k[2], k[3]);                          // k = 2
  ce(k[0], k[3]); ce(k[1], k[2]); ce(k[0], k[1]); ce(k[2], k[3]);   // k = 4: flip, j = 1
  if (P >= 8) sort_level<8>(k, s_x, base, lane);
  if (P >= 16) sort_level<16>(k, s_x, base, lane);
  if (P >= 32) sort_level<32>(k, s_x, base, lane);
  if (P >= 64) sort_level<64>(k, s_x, base, lane);
  if (P >= 128) sort_level<128>(k, s_x, base, lane);
  if (P >= 256) sort_level<256>(k, s_x, base, lane);
  if (P >= 512) sort_level<512>(k, s_x, base, lane);
  if (P >= 1024) sort_level<1024>(k, s_x, base, lane);
#pragma unroll
  for (int r = 0; r < 4; r++)
    if (base + r < n) point_list[beg + base + r] = (uint32_t)k[r];
}

// ---------------------------------------------------------------------------------------------------------
// K4, lists longer than 1024 entries - a second launch, so that the common case keeps its 8 KiB LDS footprint.
//   * up to kSortLds = 4096 entries: the list is cut into chunks of 1024 (256 threads x 4 keys).  Every chunk is sorted
//     by the register network above (levels 2 .. 1024) and parked in LDS; the remaining one or two levels of the
//     network (2048, 4096) run as their chunk-crossing stages on the LDS array (the flip, and for 4096 the half-cleaner
//     of distance 1024) followed, per chunk, by the half-cleaners 512 .. 1 in registers again.  A 4096-entry list costs
//     3 LDS stages + 4 + 8 register passes instead of the 78 LDS round trips of the plain LDS network (which this
//     replaced: 87 -> 57 us and less on the 4 x 100k-object scene of config #4, whose tiles hold 1-3 k splats);
//   * beyond: the plain network on global memory (one workgroup: its barriers order its own accesses).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void clean_chunk_1024(uint64_t (&k)[4], uint64_t *s_x, uint32_t base, int lane) {
  // the half-cleaners 512 .. 1 of a level above 1024, inside one 1024-key chunk
  cross_stage<false>(k, s_x, base, 512u, (base & 512u) == 0);
  cross_stage<false>(k, s_x, base, 256u, (base & 256u) == 0);
  lane_stage<32, false>(k, (lane & 32) == 0, lane);
  lane_stage<16, false>(k, (lane & 16) == 0, lane);
  lane_stage<8, false>(k, (lane & 8) == 0, lane);
  lane_stage<4, false>(k, (lane & 4) == 0, lane);
  lane_stage<2, false>(k, (lane & 2) == 0, lane);
  lane_stage<1, false>(k, (lane & 1) == 0, lane);
  thread_tail(k);
}

__device__ __forceinline__ void sort_long_tile(int tile, const uint32_t *__restrict__ tile_start, uint64_t *__restrict__ keys,
                                               uint32_t *__restrict__ point_list, uint32_t capacity, uint64_t *s_keys, uint64_t *s_x) {
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const TileRange tr = tile_range(tile_start, tile, capacity);
  const uint32_t beg = tr.beg, n = tr.end - tr.beg;
  if (n <= 1024) return;   // sort_tiles_reg_kernel's
  uint32_t P = 2048;
  while (P < n) P <<= 1;
  if (n > (uint32_t)kSortLds) {
    bitonic_sort(keys + beg, n, P);
    for (uint32_t i = threadIdx.x; i < n; i += 256) point_list[beg + i] = (uint32_t)keys[beg + i];
    return;
  }
  const uint32_t base = 4 * threadIdx.x;
  const int lane = threadIdx.x & 63;
  constexpr uint64_t kInf = ~0ull;
  uint64_t k[4];
  auto park = [&](uint32_t c) {
    u64x2 w0, w1;
    w0.x = k[0]; w0.y = k[1]; w1.x = k[2]; w1.y = k[3];
    u64x2 *dst = reinterpret_cast<u64x2 *>(s_keys + c + base);
    dst[0] = w0; dst[1] = w1;
  };
  auto fetch = [&](uint32_t c) {
    const u64x2 *src = reinterpret_cast<const u64x2 *>(s_keys + c + base);
    const u64x2 w0 = src[0], w1 = src[1];
    k[0] = w0.x; k[1] = w0.y; k[2] = w1.x; k[3] = w1.y;
  };
  for (uint32_t c = 0; c < P; c += 1024) {   // levels 2 .. 1024, chunk by chunk, in registers
#pragma unroll
    for (int r = 0; r < 4; r++) k[r] = c + base + r < n ? keys[beg + c + base + r] : kInf;
    if (c < n) {   // (a chunk of nothing but padding is sorted as it is)
      uint32_t Pc = 4;   // the last chunk's network only as large as its real entries need: the padding never moves
      while (Pc < n - c && Pc < 1024) Pc <<= 1;
      ce(k[0], k[1]); ce(k[2], k[3]);
      ce(k[0], k[3]); ce(k[1], k[2]); ce(k[0], k[1]); ce(k[2], k[3]);
      if (Pc >= 8) sort_level<8>(k, s_x, base, lane);
      if (Pc >= 16) sort_level<16>(k, s_x, base, lane);
      if (Pc >= 32) sort_level<32>(k, s_x, base, lane);
      if (Pc >= 64) sort_level<64>(k, s_x, base, lane);
      if (Pc >= 128) sort_level<128>(k, s_x, base, lane);
      if (Pc >= 256) sort_level<256>(k, s_x, base, lane);
      if (Pc >= 512) sort_level<512>(k, s_x, base, lane);     // (workgroup-uniform: these two hold barriers)
      if (Pc >= 1024) sort_level<1024>(k, s_x, base, lane);
    }
    park(c);
  }
  for (uint32_t K = 2048; K <= P; K <<= 1) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (P >> 1); i += 256) {   // flip: lo <-> mirrored partner inside each K-block
      const uint32_t lo = (i / (K >> 1)) * K + (i & ((K >> 1) - 1)), hi = lo ^ (K - 1);
      const uint64_t u = s_keys[lo], v = s_keys[hi];
      if (u > v) { s_keys[lo] = v; s_keys[hi] = u; }
    }
    if (K == 4096) {
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < (P >> 1); i += 256) {   // half-cleaner of distance 1024
        const uint32_t lo = ((i >> 10) << 11) + (i & 1023u), hi = lo + 1024;
        const uint64_t u = s_keys[lo], v = s_keys[hi];
        if (u > v) { s_keys[lo] = v; s_keys[hi] = u; }
      }
    }
    __syncthreads();
    for (uint32_t c = 0; c < n; c += 1024) {   // (chunks at or above n hold padding only, before and after)
      fetch(c);
      clean_chunk_1024(k, s_x, base, lane);
      if (K == P) {   // last level: straight out
#pragma unroll
        for (int r = 0; r < 4; r++)
          if (c + base + r < n) point_list[beg + c + base + r] = (uint32_t)k[r];
      } else {
        park(c);
      }
    }
  }
}

// A fixed, small grid walks the list of long tiles the register kernel left (header->long_tiles ids in long_list): with
// no long tile - the usual case - its workgroups read one word and leave, instead of one workgroup per tile doing so.
__global__ void __launch_bounds__(256)
sort_tiles_long_kernel(const uint32_t *__restrict__ tile_start, uint64_t *__restrict__ keys, uint32_t *__restrict__ point_list,
                       uint32_t capacity, const uint32_t *__restrict__ long_list, const StateHeader *__restrict__ header) {
  __shared__ __attribute__((aligned(16))) uint64_t s_keys[kSortLds];
  __shared__ __attribute__((aligned(16))) uint64_t s_x[1024];
  const uint32_t count = header->long_tiles;
  for (uint32_t k = blockIdx.x; k < count; k += gridDim.x) {
    sort_long_tile((int)long_list[k], tile_start, keys, point_list, capacity, s_keys, s_x);
    __syncthreads();   // the next tile reuses the staging arrays
  }
}

// ---------------------------------------------------------------------------------------------------------
// Deterministic mode.  The rows are addressed by the (Gaussian, tile) pair's ordinal in Gaussian-major order, so the rows
// of one Gaussian are CONTIGUOUS - partial[4 * pair_base[i] ... 4 * pair_base[i + 1]) - and the ordered per-Gaussian sum
// is a streaming read with no search (round 3 found a Gaussian's row in every block's depth-sorted hit list by binary
// search: ~190 dependent loads per Gaussian, 2.7 ms of a 3.5 ms view).
//   pair_count_kernel / pair_base_kernel : pair_base[i] = number of (Gaussian, tile) pairs of the Gaussians before i
//                                          (a two-level exclusive scan of the tile counts the binning used)
//   reduce_pair_rows_kernel              : kLanes lanes per Gaussian (lane = float of a row) add the flagged rows in the
//                                          fixed order tiles of the mask x blocks 0..3 (the 3-D rows and the 2-D ones)
// ---------------------------------------------------------------------------------------------------------
constexpr int kScanBlock = kPairScanBlock;   // Gaussians per workgroup of the pair-count scan
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t *s_red) {   // 256 threads
  for (int off = 32; off >= 1; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}
__global__ void __launch_bounds__(256)
pair_count_kernel(int N, const BinRec *__restrict__ bin, const uint64_t *__restrict__ tile_mask, uint32_t *__restrict__ block_sums) {
  __shared__ uint32_t s_red[4];
  uint32_t v = 0;
  for (int k = 0; k < kScanBlock / 256; k++) {
    const int i = blockIdx.x * kScanBlock + k * 256 + threadIdx.x;
    if (i < N) {
      const uint4 raw = reinterpret_cast<const uint4 *>(bin)[i];
      v += pairs_of(*reinterpret_cast<const BinRec *>(&raw), tile_mask[i]);
    }
  }
  v = block_sum_u32(v, s_red);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = v;
}
__global__ void __launch_bounds__(256)
pair_base_kernel(int N, const BinRec *__restrict__ bin, const uint64_t *__restrict__ tile_mask,
                 const uint32_t *__restrict__ block_sums, uint32_t *__restrict__ pair_base) {
  __shared__ uint32_t s_red[4], s_wave[4];
  // the pairs of the workgroups before this one (at most ~1000 words for a million Gaussians: every workgroup adds them itself)
  uint32_t before = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += 256) before += block_sums[b];
  uint32_t run = block_sum_u32(before, s_red);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = 0; k < kScanBlock / 256; k++) {
    const int i = blockIdx.x * kScanBlock + k * 256 + threadIdx.x;
    uint32_t c = 0;
    if (i < N) {
      const uint4 raw = reinterpret_cast<const uint4 *>(bin)[i];
      c = pairs_of(*reinterpret_cast<const BinRec *>(&raw), tile_mask[i]);
    }
    uint32_t inc = c;   // inclusive prefix inside the wave
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)inc, off, 64);
      if (lane >= off) inc += o;
    }
    __syncthreads();
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    uint32_t wbase = 0;
    for (int w = 0; w < wv; w++) wbase += s_wave[w];
    if (i < N) pair_base[i] = run + wbase + inc - c;
    run += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) pair_base[N] = run;
}

// rows of kStride floats, of which the first kUsed are summed (the rest of the accumulator row is written as zeros)
template <int kStride, int kUsed, int kLanes>
__global__ void __launch_bounds__(256)
reduce_pair_rows_kernel(int N, const uint32_t *__restrict__ pair_base, uint32_t capacity, const uint8_t *__restrict__ row_flags,
                        const float *__restrict__ partial, float *__restrict__ acc) {
  const int i = blockIdx.x * (256 / kLanes) + (threadIdx.x / kLanes), col = threadIdx.x % kLanes;
  if (i >= N || col >= kStride) return;
  const uint32_t r0 = min(pair_base[i], capacity) * 4u, r1 = min(pair_base[i + 1], capacity) * 4u;
  float sum = 0.0f;
  // four (Gaussian, tile) pairs = sixteen rows per step: the four flag words first, then every flagged row, all loads in
  // flight together (a Gaussian has 2.4 pairs on average: one step); the additions keep the fixed order pair, block
  for (uint32_t r = r0; r < r1; r += 16) {
    uint32_t f[4];
#pragma unroll
    for (int p = 0; p < 4; p++) f[p] = r + 4 * p < r1 ? *reinterpret_cast<const uint32_t *>(row_flags + r + 4 * p) : 0u;
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const bool on = (f[k >> 2] >> (8 * (k & 3))) & 0xFFu;
      v[k] = on ? partial[(size_t)(r + k) * kStride + col] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 16; k++) sum += v[k];   // (an absent row adds an exact zero)
  }
  acc[(size_t)i * kStride + col] = col < kUsed ? sum : 0.0f;
}

}  // namespace

int bin_count_and_scan(const StateLayout &L, char *base, int N, int debug, hipStream_t stream) {
  uint32_t *tile_count = (uint32_t *)(base + L.tile_count);
  if (L.two_level) {
    // first level: the bins are cells (one pass, the histogram matrix is nb x cells); the totals land in tile_count[0 .. cells)
    const int per_block = (max(N, 1) + L.nb - 1) / L.nb;
    uint32_t *block_hist = (uint32_t *)(base + L.block_hist);
    {
      ProfScope prof(kKCountTiles, stream);
      count_tiles_lds_kernel<true><<<L.nb, kBinThreads, (size_t)L.cells * 4, stream>>>(
          N, per_block, L.nb, L.cells, -1, (const BinRec *)(base + L.bin), (const uint64_t *)(base + L.tile_mask), L.cells, L.cells_x,
          block_hist, (StateHeader *)(base + L.header));
      scan_block_hist_kernel<<<(L.cells + kScanTiles - 1) / kScanTiles, kScanTiles * kScanSegs, 0, stream>>>(
          L.nb, L.cells, block_hist, tile_count, (StateHeader *)(base + L.header));
    }
    SCORP_KERNEL_CHECK("count_cells", debug, stream);
    return SCORP_OK;
  }
  if (L.lds_binning) {
    const int per_block = (max(L.bin_n() >= 0 ? L.bin_n() : N, 1) + L.nb - 1) / L.nb;
    uint32_t *block_hist = (uint32_t *)(base + L.block_hist);
    {
      ProfScope prof(kKCountTiles, stream);
      const int tpp = L.tiles_per_pass();
      // histograms above 64 KiB need the kernels' dynamic-LDS limit raised.  The attribute is PER DEVICE (a process that
      // drives a second GPU must set it there too), so it is set whenever such a launch is about to happen - two cheap
      // host calls, no process-global flag, no data race between threads - and its result is checked.
      if ((size_t)tpp * 4 > 64 * 1024) {
        SCORP_HIP_CHECK(hipFuncSetAttribute((const void *)count_tiles_lds_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsTiles * 4));
        SCORP_HIP_CHECK(hipFuncSetAttribute((const void *)scatter_pairs_lds_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsTiles * 4));
      }
      count_tiles_lds_kernel<false><<<L.nb * L.bin_passes(), kBinThreads, (size_t)tpp * 4, stream>>>(
          N, per_block, L.nb, tpp, L.bin_n(), (const BinRec *)(base + L.bin), (const uint64_t *)(base + L.tile_mask), L.tiles, L.tiles_x,
          block_hist, L.scan_in_scatter() ? (StateHeader *)(base + L.header) : nullptr);
      scan_block_hist_kernel<<<(L.tiles + kScanTiles - 1) / kScanTiles, kScanTiles * kScanSegs, 0, stream>>>(
          L.nb, L.tiles, block_hist, tile_count, L.scan_in_scatter() ? (StateHeader *)(base + L.header) : nullptr);
    }
    SCORP_KERNEL_CHECK("count_tiles", debug, stream);
  }
  if (!L.scan_in_scatter()) {
    ProfScope prof(kKScanTiles, stream);
    if (L.tiles > 8192 && L.tiles <= kMaxLdsTiles) {
      if ((size_t)L.tiles * 4 > 64 * 1024)
        SCORP_HIP_CHECK(hipFuncSetAttribute((const void *)scan_tiles_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsTiles * 4));
      scan_tiles_lds_kernel<<<1, 1024, (size_t)L.tiles * 4, stream>>>(tile_count, (uint32_t *)(base + L.tile_start), L.tiles,
                                                                      (StateHeader *)(base + L.header));
    } else {
      scan_tiles_kernel<<<1, 1024, 0, stream>>>(tile_count, (uint32_t *)(base + L.tile_start), L.tiles,
                                                (StateHeader *)(base + L.header));
    }
  }
  SCORP_KERNEL_CHECK("scan_tiles", debug, stream);
  return SCORP_OK;
}

int bin_scatter_and_sort(const StateLayout &L, const PairLayout &P, char *base, char *pb, int N, uint32_t capacity,
                         int debug, hipStream_t stream, uint32_t *header_copy) {
  uint32_t *tile_count = (uint32_t *)(base + L.tile_count), *tile_start = (uint32_t *)(base + L.tile_start);
  uint64_t *keys = (uint64_t *)(pb + P.keys);
  uint32_t *point_list = (uint32_t *)(pb + P.list);
  StateHeader *header = (StateHeader *)(base + L.header);
  if (L.two_level) {
    // pairs -> cell buckets (first key buffer) -> tile buckets (second key buffer), then the per-tile sort reads the second
    uint32_t *cell_start = (uint32_t *)(base + L.cell_start);
    uint64_t *keys2 = (uint64_t *)(pb + P.keys2);
    {
      ProfScope prof(kKScatterPairs, stream);
      const int per_block = (max(N, 1) + L.nb - 1) / L.nb;
      scatter_pairs_lds_kernel<true><<<L.nb, kBinThreads, (size_t)L.cells * 4, stream>>>(
          N, per_block, L.nb, L.cells, -1, (const BinRec *)(base + L.bin), (const uint64_t *)(base + L.tile_mask), L.cells, L.cells_x,
          (const uint32_t *)(base + L.block_hist), cell_start, tile_count, keys, capacity, header, header_copy);
      expand_cells_kernel<<<L.cells, kExpandThreads, 0, stream>>>(cell_start, keys, keys2, tile_start, capacity, L.cells_x, L.tiles_x, L.tiles_y);
    }
    SCORP_KERNEL_CHECK("scatter_cells", debug, stream);
    {
      ProfScope prof(kKSortTiles, stream);
      sort_tiles_reg_kernel<<<L.tiles, 256, 0, stream>>>(tile_start, keys2, point_list, capacity, tile_count, header);
      sort_tiles_long_kernel<<<L.tiles < 512 ? L.tiles : 512, 256, 0, stream>>>(tile_start, keys2, point_list, capacity, tile_count, header);
    }
    SCORP_KERNEL_CHECK("sort_tiles", debug, stream);
    return SCORP_OK;
  }
  {
    ProfScope prof(kKScatterPairs, stream);
    if (L.lds_binning) {
      const int per_block = (max(L.bin_n() >= 0 ? L.bin_n() : N, 1) + L.nb - 1) / L.nb;
      const int tpp = L.tiles_per_pass();
      scatter_pairs_lds_kernel<false><<<L.nb * L.bin_passes(), kBinThreads, (size_t)tpp * 4, stream>>>(
          N, per_block, L.nb, tpp, L.bin_n(), (const BinRec *)(base + L.bin), (const uint64_t *)(base + L.tile_mask), L.tiles, L.tiles_x,
          (const uint32_t *)(base + L.block_hist), tile_start, L.scan_in_scatter() ? tile_count : nullptr, keys, capacity,
          header, header_copy);
    } else {
      scatter_pairs_kernel<<<(max(N, 1) + 255) / 256, 256, 0, stream>>>(
          N, (const BinRec *)(base + L.bin), (const uint64_t *)(base + L.tile_mask), tile_count, tile_start, L.tiles_x,
          keys, capacity, header, header_copy);
    }
  }
  SCORP_KERNEL_CHECK("scatter_pairs", debug, stream);
  {
    ProfScope prof(kKSortTiles, stream);
    // (tile_count is dead once the pairs are scattered - the next preprocess rewrites it - and holds the long tiles' ids)
    sort_tiles_reg_kernel<<<L.tiles, 256, 0, stream>>>(tile_start, keys, point_list, capacity, tile_count, header);
    sort_tiles_long_kernel<<<L.tiles < 512 ? L.tiles : 512, 256, 0, stream>>>(tile_start, keys, point_list, capacity, tile_count, header);
  }
  SCORP_KERNEL_CHECK("sort_tiles", debug, stream);
  return SCORP_OK;
}

template <int kStride, int kUsed, int kLanes>
void launch_reduce_pair_rows(int N, const uint32_t *pair_base, uint32_t capacity, const uint8_t *row_flags,
                             const float *partial, float *acc, hipStream_t stream) {
  constexpr int per_block = 256 / kLanes;
  reduce_pair_rows_kernel<kStride, kUsed, kLanes><<<(N + per_block - 1) / per_block, 256, 0, stream>>>(
      N, pair_base, capacity, row_flags, partial, acc);
}
// 3DGS: ten floats of a 16-float row; 2DGS: the whole 20-float row (kAcc2Stride, surfel.hpp)
template void launch_reduce_pair_rows<kAccStride, 10, 16>(int, const uint32_t *, uint32_t, const uint8_t *, const float *, float *,
                                                          hipStream_t);
template void launch_reduce_pair_rows<20, 20, 32>(int, const uint32_t *, uint32_t, const uint8_t *, const float *, float *,
                                                  hipStream_t);
// the mask vote (mask_vote.hip): sixteen sums per row, all of them used
template void launch_reduce_pair_rows<16, 16, 16>(int, const uint32_t *, uint32_t, const uint8_t *, const float *, float *,
                                                  hipStream_t);

// pair_base[i] = the number of (Gaussian, tile) pairs of the Gaussians before i (pair_base[N] = all of them), from the tile
// rectangles / masks the binning used; shared by the 3-D and the 2-D deterministic backward and the mask vote (the 2-D
// state holds the same BinRec / tile-mask arrays)
int setup_pair_rows(const StateLayout &L, const void *state, int N, uint64_t capacity, int row_floats, void *scratch, int debug,
                    hipStream_t stream, PairRows *rows) {
  const DetLayout DL(N, capacity, row_floats);
  char *p = (char *)scratch;
  *rows = {(float *)(p + DL.acc), (float *)(p + DL.partial), (uint8_t *)(p + DL.flags), (uint32_t *)(p + DL.pair_base)};
  SCORP_HIP_CHECK(hipMemsetAsync(rows->flags, 0, (size_t)(capacity > 0 ? capacity : 1) * 4, stream));
  const BinRec *bin = (const BinRec *)((const char *)state + L.bin);
  const uint64_t *tile_mask = (const uint64_t *)((const char *)state + L.tile_mask);
  uint32_t *block_sums = (uint32_t *)(p + DL.block_sums);
  const int blocks = (N + kScanBlock - 1) / kScanBlock;
  pair_count_kernel<<<blocks, 256, 0, stream>>>(N, bin, tile_mask, block_sums);
  pair_base_kernel<<<blocks, 256, 0, stream>>>(N, bin, tile_mask, block_sums, rows->pair_base);
  SCORP_KERNEL_CHECK("pair_base", debug, stream);
  return SCORP_OK;
}

}  // namespace scorp

// The debug entry points' view of the tile lists: tile_start[tiles + 1] in RASTER tile order with the lists concatenated in
// that order - whatever order they have in the pair buffer (cell-major under the two-level binning).
int scorp::debug_tiles(bool mode2d, const void *state, const void *pairs, uint64_t capacity, int N, int W, int H,
                       uint32_t *tile_start, uint32_t *point_list, hipStream_t stream) {
  if (int e = check_buffers(state, pairs, capacity)) return e;
  const StateLayout L(N, W, H, mode2d);
  const PairLayout P(capacity);
  StateHeader h;
  if (int e = read_header(state, stream, &h)) return e;
  const size_t n = h.num_pairs < capacity ? h.num_pairs : (size_t)capacity;
  uint32_t *range = (uint32_t *)malloc(((size_t)L.tiles + 1) * 8), *list = (uint32_t *)malloc((n ? n : 1) * 4);
  if (!range || !list) { free(range); free(list); set_error("out of host memory"); return SCORP_ERR_INVALID; }
  hipError_t e = hipMemcpyAsync(range, (const char *)state + L.tile_start, (size_t)L.tiles * 8, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && n) e = hipMemcpyAsync(list, (const char *)pairs + P.list, n * 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { free(range); free(list); set_error("copy of the tile lists failed: %s", hipGetErrorString(e)); return SCORP_ERR_HIP; }
  uint32_t run = 0;
  for (int t = 0; t < L.tiles; t++) {
    const uint32_t b = range[2 * t] < n ? range[2 * t] : (uint32_t)n, en = range[2 * t + 1] < n ? range[2 * t + 1] : (uint32_t)n;
    if (tile_start) tile_start[t] = run;
    if (point_list && en > b) memcpy(point_list + run, list + b, (size_t)(en - b) * 4);
    run += en > b ? en - b : 0;
  }
  if (tile_start) tile_start[L.tiles] = run;
  free(range); free(list);
  return SCORP_OK;
}
