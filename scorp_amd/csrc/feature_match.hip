// feature_match.hip - the nearest target descriptor of every source descriptor, by brute force (rule M1 of the global-
// registration block of include/scorp_gs.h; scorp_amd/global_registration.py: match_features).  Rows are 33 fp32 values,
// the FPFH descriptor rounded once; D2(a, b) is the float64 sum over k = 0 .. 32 in ascending order from 0.0 of
// (double(a_k) - double(b_k))^2, product and sum each rounded on its own, and the target row of smallest (D2, index) wins.
//
//   match    one thread per source row, its 33 values in registers as doubles.  Target rows pass through LDS in tiles of
//            kMatchTile rows, converted to float64 once on the way in; every lane reads the same address (a broadcast).
//            ns alone rarely fills the device (10^5 rows are 391 workgroups on 256 CUs, 2 * 10^4 are 79), so the tiles of
//            the target are split over blockIdx.y: each split leaves its best (D2, index) per source row in the workspace.
//   merge    one thread per source row takes the smallest (D2, index) of its splits.  Always run, also for one split: one
//            path.  No atomics anywhere.
#include "common.hpp"

#pragma clang fp contract(off)

namespace scorp {
namespace {

constexpr int kMatchDim = 33;
constexpr int kMatchThreads = 256;
constexpr int kMatchTile = 64;            // target rows per LDS tile
constexpr int kMatchRowStride = 34;       // doubles per row in LDS: 16-byte aligned rows
constexpr int kMatchWantBlocks = 1024;    // four workgroups per CU

// The target split of a call: `tiles` tiles per blockIdx.y, `splits` of them.  A function of (ns, nt) alone.
struct MatchSplit {
  int64_t tiles, splits;
  MatchSplit(int64_t ns, int64_t nt) {
    const int64_t bx = (ns + kMatchThreads - 1) / kMatchThreads, ntiles = (nt + kMatchTile - 1) / kMatchTile;
    int64_t want = kMatchWantBlocks / (bx > 0 ? bx : 1);
    want = want < 1 ? 1 : (want > ntiles ? ntiles : want);
    if (want > 65535) want = 65535;
    tiles = (ntiles + want - 1) / want;
    if (tiles < 1) tiles = 1;
    splits = (ntiles + tiles - 1) / tiles;
    if (splits < 1) splits = 1;
  }
};

__global__ void __launch_bounds__(kMatchThreads) feature_match_kernel(const float *__restrict__ src, const float *__restrict__ tgt, int ns, int nt,
                                                                      int tiles_per_split, double *__restrict__ part_d2,
                                                                      int32_t *__restrict__ part_idx) {
  __shared__ __attribute__((aligned(16))) double tile[kMatchTile * kMatchRowStride];
  const int i = blockIdx.x * kMatchThreads + threadIdx.x;
  const bool live = i < ns;
  double a[kMatchDim];
#pragma unroll
  for (int k = 0; k < kMatchDim; k++) a[k] = live ? (double)src[(size_t)i * kMatchDim + k] : 0.0;
  double best = __builtin_inf();
  int32_t bidx = -1;
  const int64_t row0 = (int64_t)blockIdx.y * tiles_per_split * kMatchTile;
  const int64_t row1 = row0 + (int64_t)tiles_per_split * kMatchTile < nt ? row0 + (int64_t)tiles_per_split * kMatchTile : nt;
  for (int64_t base = row0; base < row1; base += kMatchTile) {
    const int rows = (int)(row1 - base < kMatchTile ? row1 - base : kMatchTile);
    __syncthreads();   // (the tile of the round before has been read)
    for (int e = threadIdx.x; e < rows * kMatchDim; e += kMatchThreads)
      tile[e / kMatchDim * kMatchRowStride + e % kMatchDim] = (double)tgt[(size_t)base * kMatchDim + e];
    __syncthreads();
    if (live) {
      for (int r = 0; r < rows; r++) {
        const double *__restrict__ b = tile + r * kMatchRowStride;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < kMatchDim; k++) {
          const double d = a[k] - b[k];
          acc = acc + d * d;
        }
        if (acc < best) { best = acc; bidx = (int32_t)(base + r); }   // (rows ascend: a tie keeps the lower index)
      }
    }
  }
  if (live) {
    part_d2[(size_t)blockIdx.y * ns + i] = best;
    part_idx[(size_t)blockIdx.y * ns + i] = bidx;
  }
}

__global__ void __launch_bounds__(kMatchThreads) feature_match_merge_kernel(const double *__restrict__ part_d2, const int32_t *__restrict__ part_idx,
                                                                            int ns, int splits, int32_t *__restrict__ out_index,
                                                                            double *__restrict__ out_d2) {
  const int i = blockIdx.x * kMatchThreads + threadIdx.x;
  if (i >= ns) return;
  double best = part_d2[i];
  int32_t bidx = part_idx[i];
  for (int s = 1; s < splits; s++) {
    const double d = part_d2[(size_t)s * ns + i];
    const int32_t id = part_idx[(size_t)s * ns + i];
    if (id >= 0 && (bidx < 0 || d < best || (d == best && id < bidx))) { best = d; bidx = id; }
  }
  out_index[i] = bidx;
  out_d2[i] = best;
}

size_t match_part_bytes(int64_t ns, int64_t splits) { return align_up((size_t)ns * splits * 8, 256); }

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int32_t scorp_feature_match_tile_rows(void) { return kMatchTile; }

extern "C" int32_t scorp_feature_match_split_rows(int32_t ns, int32_t nt) {
  return (int32_t)(MatchSplit(ns > 0 ? ns : 1, nt > 0 ? nt : 1).tiles * kMatchTile);
}

extern "C" size_t scorp_feature_match_workspace_bytes(int32_t ns, int32_t nt) {
  const int64_t s = ns > 0 ? ns : 1;
  const int64_t splits = MatchSplit(s, nt > 0 ? nt : 1).splits;
  return match_part_bytes(s, splits) + align_up((size_t)s * splits * 4, 256);
}

extern "C" int scorp_feature_match(const float *src, int32_t ns, const float *tgt, int32_t nt, int32_t *out_index, double *out_d2,
                                   void *workspace, size_t workspace_bytes, scorp_stream_t stream) {
  if (ns < 1 || nt < 1) { set_error("feature_match: empty source or target"); return SCORP_ERR_INVALID; }
  if (ns > (1 << 30) || nt > (1 << 30)) { set_error("feature_match: more than 2^30 rows"); return SCORP_ERR_INVALID; }
  if (!src || !tgt || !out_index || !out_d2) { set_error("feature_match: NULL argument"); return SCORP_ERR_INVALID; }
  const size_t need = scorp_feature_match_workspace_bytes(ns, nt);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 255)) {
    set_error("feature_match: workspace NULL, too small or not 256-byte aligned (%zu < %zu)", workspace_bytes, need);
    return SCORP_ERR_INVALID;
  }
  const MatchSplit S(ns, nt);
  double *part_d2 = (double *)workspace;
  int32_t *part_idx = (int32_t *)((char *)workspace + match_part_bytes(ns, S.splits));
  hipStream_t s = (hipStream_t)stream;
  const unsigned bx = (unsigned)((ns + kMatchThreads - 1) / kMatchThreads);
  feature_match_kernel<<<dim3(bx, (unsigned)S.splits), kMatchThreads, 0, s>>>(src, tgt, ns, nt, (int)S.tiles, part_d2, part_idx);
  SCORP_KERNEL_CHECK("feature_match", 0, s);
  feature_match_merge_kernel<<<bx, kMatchThreads, 0, s>>>(part_d2, part_idx, ns, (int)S.splits, out_index, out_d2);
  SCORP_KERNEL_CHECK("feature_match_merge", 0, s);
  return SCORP_OK;
}
