// tsdf_blocks.hip — the bounded TSDF route: a sparse volume of 16^3-voxel blocks that exist only near the observed surface
// (what gs2dgs/utils/mesh_utils.py:138-180 extract_mesh_bounded asks of Open3D's ScalableTSDFVolume).  The rules - voxel
// centres, block keys, which blocks a view touches, the nearest-pixel projective update - are written down in
// include/scorp_gs.h and are the specification; tests/tsdf_blocks_reference.py restates them in numpy float64.  Nothing here
// was compared with Open3D's own output.
//
// Three calls, the caller's compaction (keys != empty, sort, gather) between the first and the other two:
//   touch      one lane per sampled pixel, the view in blockIdx.y (its 16 numbers come through a uniform address).  The
//              up to 27 blocks round the back-projected point are inserted into an open-addressing table of 64-bit keys:
//              a slot is claimed by ONE compare-and-swap, the view's bit is set by atomicOr.  Neighbouring pixels insert
//              the same keys and set the same bit over and over, so a lane first LOOKS (agent-scope relaxed atomic loads:
//              the values are rewritten by other CUs' atomics while the kernel runs) and issues the atomic only when the
//              slot is still empty / the bit still clear: after the first arrival the rest is read traffic.  Probing is
//              linear and bounded by the table's size; a full table sets a bit of the caller's overflow word and drops the
//              insert, and every insert after that is dropped unprobed (the caller discards the table and repeats).  Nothing waits on another lane.  Which slot a key lands in depends on the order of arrival; the SET
//              of keys and their masks do not, and the caller sorts.
//   neighbors  nbr[b, 27]: the rank of every adjacent block by binary search in the sorted keys, -1 where there is none.
//   integrate  one 256-thread workgroup per block; lane t owns the voxels t, t + 256, ... (local x = 0 .. 15 at the lane's
//              fixed (y, z)), so every store is coalesced.  The view loop is inside and wave-uniform, the mask test is
//              block-uniform (scalar), a voxel's tsdf / w / colour stay in registers over all views and are stored once.
// No LDS, no scratch.  The arithmetic is compiled without fp contraction: every product and sum rounds on its own, as the
// numpy float32 restatement rounds.
#include "lattice.hpp"

namespace scorp {
namespace {

constexpr uint64_t kBlkEmpty = ~(uint64_t)0;   // no block has it: a key is below 2^63

struct BlkViews {
  const float *depth;
  const uint8_t *rgb;
  const float *cam;   // [V, 16]: E row-major (12), fx, fy, cx, cy
  int V, W, H;
};

__global__ void __launch_bounds__(kBlkThreads) blocks_clear_kernel(uint64_t *__restrict__ keys, uint32_t *__restrict__ view_mask,
                                                                   uint64_t slots, uint64_t mask_words, uint32_t *__restrict__ overflow) {
  // grid-stride: 2^32 slots times the mask words of many views is more than a grid of 256-thread blocks can number
  const uint64_t first = (uint64_t)blockIdx.x * kBlkThreads + threadIdx.x, step = (uint64_t)gridDim.x * kBlkThreads;
  for (uint64_t i = first; i < mask_words; i += step) {
    if (i < slots) keys[i] = kBlkEmpty;
    view_mask[i] = 0u;
  }
  if (first == 0) *overflow = 0u;
}

__global__ void __launch_bounds__(kBlkThreads) blocks_touch_kernel(const BlkViews a, int stride, int su, int sv, float block_len,
                                                                   float trunc, uint64_t *keys, uint32_t *view_mask,
                                                                   uint64_t slot_mask, int words, uint32_t *overflow) {
#pragma clang fp contract(off)
  const int view = blockIdx.y;   // uniform: the view's numbers are scalar loads
  const uint32_t p = blockIdx.x * kBlkThreads + threadIdx.x;
  if (p >= (uint32_t)su * (uint32_t)sv) return;
  const int u = (int)(p % (uint32_t)su) * stride, v = (int)(p / (uint32_t)su) * stride;
  const float d = a.depth[((size_t)view * a.H + v) * a.W + u];
  if (!(d > 0.0f)) return;
  const float *__restrict__ C = a.cam + (size_t)view * 16;
  const float fx = C[12], fy = C[13], cx = C[14], cy = C[15];
  const float qx = ((float)u - cx) * d / fx - C[3], qy = ((float)v - cy) * d / fy - C[7], qz = d - C[11];
  const float w[3] = {(C[0] * qx + C[4] * qy) + C[8] * qz, (C[1] * qx + C[5] * qy) + C[9] * qz, (C[2] * qx + C[6] * qy) + C[10] * qz};
  int32_t lo[3], hi[3];
  bool in_range = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float l = floorf((w[k] - trunc) / block_len), h = floorf((w[k] + trunc) / block_len);
    in_range = in_range && l >= -(float)kBlkBias && h < (float)kBlkBias;   // (a NaN compares false)
    lo[k] = (int32_t)fminf(fmaxf(l, -(float)kBlkBias), (float)(kBlkBias - 1));
    hi[k] = (int32_t)fminf(fmaxf(h, -(float)kBlkBias), (float)(kBlkBias - 1));
  }
  if (!in_range) { atomicOr(overflow, 2u); return; }
  // sdf_trunc <= 16 voxel_length: at most 3 blocks per axis; the clamp keeps the loops short whatever the floats were
  hi[0] = min(hi[0], lo[0] + 2); hi[1] = min(hi[1], lo[1] + 2); hi[2] = min(hi[2], lo[2] + 2);
  const uint32_t bit = 1u << (view & 31);
  for (int32_t bx = lo[0]; bx <= hi[0]; bx++)
    for (int32_t by = lo[1]; by <= hi[1]; by++)
      for (int32_t bz = lo[2]; bz <= hi[2]; bz++) {
        // A full table is discarded by the caller, so once some lane has found it full nobody probes it again: without this
        // look every later insert of an absent key would walk all num_slots slots before giving up.
        if (__hip_atomic_load(overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 1u) return;
        const uint64_t key = blk_key(bx, by, bz);
        uint64_t slot = mix64(key) & slot_mask;
        bool done = false;
        for (uint64_t probe = 0; probe <= slot_mask; probe++) {
          uint64_t cur = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (cur == kBlkEmpty) {
            cur = atomicCAS((unsigned long long *)(keys + slot), (unsigned long long)kBlkEmpty, (unsigned long long)key);
            if (cur == kBlkEmpty) cur = key;
          }
          if (cur == key) {
            uint32_t *word = view_mask + slot * (uint64_t)words + (uint32_t)(view >> 5);
            if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
            done = true;
            break;
          }
          slot = (slot + 1) & slot_mask;
        }
        if (!done) atomicOr(overflow, 1u);
      }
}

__global__ void __launch_bounds__(kBlkThreads) blocks_neighbors_kernel(const uint64_t *__restrict__ block_keys, int32_t B,
                                                                       int32_t *__restrict__ nbr) {
  const int64_t i = (int64_t)blockIdx.x * kBlkThreads + threadIdx.x;
  if (i >= (int64_t)B * 27) return;
  const int32_t b = (int32_t)(i / 27), n = (int32_t)(i - (int64_t)b * 27);
  int32_t bx, by, bz;
  blk_coords(block_keys[b], bx, by, bz);
  bx += n / 9 - 1; by += (n / 3) % 3 - 1; bz += n % 3 - 1;
  int32_t r = -1;
  if (bx >= -kBlkBias && bx < kBlkBias && by >= -kBlkBias && by < kBlkBias && bz >= -kBlkBias && bz < kBlkBias) {
    const uint64_t key = blk_key(bx, by, bz);
    int32_t lo = 0, hi = B;   // the first rank whose key is >= key
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (block_keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    if (lo < B && block_keys[lo] == key) r = lo;
  }
  nbr[i] = r;
}

__global__ void __launch_bounds__(kBlkThreads) blocks_integrate_kernel(const BlkViews a, float voxel_length, float trunc, float u_max,
                                                                       float v_max, const uint64_t *__restrict__ block_keys,
                                                                       const uint32_t *__restrict__ view_mask, int words,
                                                                       float *__restrict__ out_tsdf, float *__restrict__ out_weight,
                                                                       float *__restrict__ out_colour) {
#pragma clang fp contract(off)
  const bool kRgb = out_colour != nullptr;   // (uniform: a kernel argument)
  const int32_t b = blockIdx.x;
  int32_t bx, by, bz;
  blk_coords(block_keys[b], bx, by, bz);
  const uint32_t *__restrict__ mask = view_mask + (size_t)b * words;   // uniform address: scalar loads
  const int t = threadIdx.x;
  const float y = voxel_length * ((float)(by * kBlkSide + (t >> 4)) + 0.5f);
  const float z = voxel_length * ((float)(bz * kBlkSide + (t & 15)) + 0.5f);
  const size_t hw = (size_t)a.W * a.H;
  for (int j = 0; j < kBlkSide; j++) {
    const float x = voxel_length * ((float)(bx * kBlkSide + j) + 0.5f);
    float tsdf = 0.0f, w = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
    for (int view = 0; view < a.V; view++) {
      if (!((mask[view >> 5] >> (view & 31)) & 1u)) continue;   // block-uniform
      const float *__restrict__ C = a.cam + (size_t)view * 16;   // uniform address: scalar loads
      const float pz = ((C[8] * x + C[9] * y) + C[10] * z) + C[11];
      if (!(pz > 0.0f)) continue;
      const float px = ((C[0] * x + C[1] * y) + C[2] * z) + C[3];
      const float py = ((C[4] * x + C[5] * y) + C[6] * z) + C[7];
      const float fx = C[12], fy = C[13], cx = C[14], cy = C[15];
      const float uf = (px * fx / pz + cx) + 0.5f, vf = (py * fy / pz + cy) + 0.5f;
      if (!(uf >= 1e-4f && uf < u_max && vf >= 1e-4f && vf < v_max)) continue;   // (a NaN compares false)
      const int u = (int)uf, v = (int)vf;
      const size_t pix = (size_t)view * hw + (size_t)v * a.W + u;
      const float d = a.depth[pix];
      if (!(d > 0.0f)) continue;
      const float rx = ((float)u - cx) / fx, ry = ((float)v - cy) / fy;
      const float sdf = (d - pz) * sqrtf((rx * rx + ry * ry) + 1.0f);
      if (!(sdf > -trunc)) continue;
      const float s = fminf(1.0f, sdf / trunc);
      const float wp = w + 1.0f;
      tsdf = (tsdf * w + s) / wp;
      if (kRgb) {
        const uint8_t *__restrict__ c = a.rgb + pix * 3;
        cr = (cr * w + (float)c[0]) / wp;
        cg = (cg * w + (float)c[1]) / wp;
        cb = (cb * w + (float)c[2]) / wp;
      }
      w = wp;
    }
    const size_t o = (size_t)b * kBlkVoxels + (size_t)j * 256 + t;
    out_tsdf[o] = tsdf;
    out_weight[o] = w;
    if (kRgb) { out_colour[o * 3 + 0] = cr; out_colour[o * 3 + 1] = cg; out_colour[o * 3 + 2] = cb; }
  }
}

int check_block_views(const ScorpTsdfBlockViews *v, const char *what) {
  if (!v || !v->depth || !v->cam) { set_error("%s: NULL views, depth or cam", what); return SCORP_ERR_INVALID; }
  if (v->num_views < 1) { set_error("%s: num_views < 1", what); return SCORP_ERR_INVALID; }
  if (v->num_views > 65535) { set_error("%s: more than 65535 views", what); return SCORP_ERR_INVALID; }
  if (v->width < 1 || v->height < 1) { set_error("%s: width and height must be at least 1", what); return SCORP_ERR_INVALID; }
  return SCORP_OK;
}

int check_block_lengths(float voxel_length, float sdf_trunc, const char *what) {
  if (!(voxel_length > 0.0f)) { set_error("%s: voxel_length must be positive", what); return SCORP_ERR_INVALID; }
  if (!(sdf_trunc > 0.0f) || !(sdf_trunc <= 16.0f * voxel_length)) {
    set_error("%s: sdf_trunc must be in (0, 16 voxel_length]", what); return SCORP_ERR_INVALID;
  }
  return SCORP_OK;
}

inline unsigned blk_grid(uint64_t n) { return (unsigned)((n + kBlkThreads - 1) / kBlkThreads); }

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_tsdf_blocks_touch(const ScorpTsdfBlockViews *views, float voxel_length, float sdf_trunc, int32_t stride,
                                       uint64_t *keys, uint32_t *view_mask, uint64_t num_slots, uint32_t *overflow,
                                       scorp_stream_t stream) {
  if (int e = check_block_views(views, "tsdf_blocks_touch")) return e;
  if (int e = check_not_null({keys, view_mask, overflow}, "tsdf_blocks_touch", "argument")) return e;
  if (stride < 1) { set_error("tsdf_blocks_touch: stride < 1"); return SCORP_ERR_INVALID; }
  if (int e = check_block_lengths(voxel_length, sdf_trunc, "tsdf_blocks_touch")) return e;
  if (num_slots == 0 || (num_slots & (num_slots - 1)) != 0 || num_slots > ((uint64_t)1 << 32)) {
    set_error("tsdf_blocks_touch: num_slots must be a power of two, at most 2^32"); return SCORP_ERR_INVALID;
  }
  const int words = (views->num_views + 31) / 32;
  const int su = (views->width + stride - 1) / stride, sv = (views->height + stride - 1) / stride;
  if ((uint64_t)su * (uint64_t)sv > (uint64_t)0x7FFFFFFF) { set_error("tsdf_blocks_touch: more than 2^31 - 1 sampled pixels per view"); return SCORP_ERR_INVALID; }
  hipStream_t s = (hipStream_t)stream;
  const uint64_t mask_words = num_slots * (uint64_t)words;
  const uint64_t clear_blocks = (mask_words + kBlkThreads - 1) / kBlkThreads;
  blocks_clear_kernel<<<(unsigned)(clear_blocks < 65536 ? clear_blocks : 65536), kBlkThreads, 0, s>>>(keys, view_mask, num_slots, mask_words,
                                                                                                   overflow);
  SCORP_KERNEL_CHECK("blocks_clear", 0, s);
  BlkViews a{views->depth, views->rgb, views->cam, views->num_views, views->width, views->height};
  blocks_touch_kernel<<<dim3(blk_grid((uint64_t)su * sv), (unsigned)views->num_views), kBlkThreads, 0, s>>>(
      a, stride, su, sv, 16.0f * voxel_length, sdf_trunc, keys, view_mask, num_slots - 1, words, overflow);
  SCORP_KERNEL_CHECK("blocks_touch", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_tsdf_blocks_neighbors(const uint64_t *block_keys, int64_t num_blocks, int32_t *out_nbr, scorp_stream_t stream) {
  if (int e = check_not_null({block_keys, out_nbr}, "tsdf_blocks_neighbors", "argument")) return e;
  if (int e = check_num_blocks(num_blocks, "tsdf_blocks_neighbors")) return e;
  hipStream_t s = (hipStream_t)stream;
  blocks_neighbors_kernel<<<blk_grid((uint64_t)num_blocks * 27), kBlkThreads, 0, s>>>(block_keys, (int32_t)num_blocks, out_nbr);
  SCORP_KERNEL_CHECK("blocks_neighbors", 0, s);
  return SCORP_OK;
}

extern "C" int scorp_tsdf_blocks_integrate(const ScorpTsdfBlockViews *views, float voxel_length, float sdf_trunc,
                                           const uint64_t *block_keys, const uint32_t *view_mask, int64_t num_blocks,
                                           float *out_tsdf, float *out_weight, float *out_colour, scorp_stream_t stream) {
  if (int e = check_block_views(views, "tsdf_blocks_integrate")) return e;
  if (int e = check_not_null({block_keys, view_mask, out_tsdf, out_weight}, "tsdf_blocks_integrate", "argument")) return e;
  if (out_colour && !views->rgb) { set_error("tsdf_blocks_integrate: out_colour without views->rgb"); return SCORP_ERR_INVALID; }
  if (int e = check_block_lengths(voxel_length, sdf_trunc, "tsdf_blocks_integrate")) return e;
  if (int e = check_num_blocks(num_blocks, "tsdf_blocks_integrate")) return e;
  BlkViews a{views->depth, views->rgb, views->cam, views->num_views, views->width, views->height};
  const int words = (views->num_views + 31) / 32;
  const float u_max = (float)views->width - 1e-4f, v_max = (float)views->height - 1e-4f;
  hipStream_t s = (hipStream_t)stream;
  blocks_integrate_kernel<<<(unsigned)num_blocks, kBlkThreads, 0, s>>>(a, voxel_length, sdf_trunc, u_max, v_max, block_keys, view_mask,
                                                                       words, out_tsdf, out_weight, out_colour);
  SCORP_KERNEL_CHECK("blocks_integrate", 0, s);
  return SCORP_OK;
}
