// tsdf.hip — multi-view TSDF fusion (gs2dgs/utils/mesh_utils.py:196-247: compute_sdf_perframe and
// compute_unbounded_tsdf) in one pass over the samples.
//
// The reference evaluates one view at a time over a chunk of samples: a matmul, two grid_samples and six masked gathers /
// scatters per (chunk, view), with the running tsdfs / weights / rgbs arrays read and written back every view.  Here a
// lane owns one sample and walks the views itself:
//   * tsdf, w and rgb live in registers for the whole view loop; every output is stored once;
//   * the view loop is wave-uniform: the 16 floats of a view's matrix come through a const __restrict__ pointer at a
//     uniform address (scalar loads), the map base of the view is scalar arithmetic;
//   * a lane outside the view's frustum skips its gathers;
//   * samples are numbered with z fastest, so the lanes of a wave project to neighbouring pixels and their four-corner
//     gathers share cache lines.
// No LDS, no atomics, no scratch.  The arithmetic is the reference's, statement for statement, in fp32; the update of
// the running means is compiled without fp contraction so that it rounds where the reference's separate kernels round.
#include "common.hpp"

namespace scorp {
namespace {

constexpr int kTsdfThreads = 256;

struct TsdfArgs {
  const float *xyz, *x, *y, *z;
  int V, W, H;
  int ny, nz;
  uint64_t first, end;
  float trunc0;   // 5 voxel_size
  float cx, cy, cz, radius;
};

// One corner of the bilinear sample: inside the map (a corner past the last row / column has weight 0 and is not read)
__device__ __forceinline__ float corner(const float *__restrict__ map, int x, int y, int W, int H) {
  return (x < W && y < H) ? map[(size_t)y * W + x] : 0.0f;
}

template <bool kRgb, bool kContracted>
__global__ void __launch_bounds__(kTsdfThreads) tsdf_fuse_kernel(const TsdfArgs a, const float *__restrict__ proj,
                                                                 const float *__restrict__ depth,
                                                                 const float *__restrict__ rgb,
                                                                 float *__restrict__ out_tsdf,
                                                                 float *__restrict__ out_rgb) {
#pragma clang fp contract(off)
  const uint64_t g = a.first + (uint64_t)blockIdx.x * kTsdfThreads + threadIdx.x;
  if (g >= a.end) return;
  float sx, sy, sz;
  if (a.xyz) {
    sx = a.xyz[g * 3 + 0]; sy = a.xyz[g * 3 + 1]; sz = a.xyz[g * 3 + 2];
  } else {
    const uint64_t t = g / (uint32_t)a.nz, iz = g - t * (uint32_t)a.nz;
    const uint64_t ix = t / (uint32_t)a.ny, iy = t - ix * (uint32_t)a.ny;
    sx = a.x[ix]; sy = a.y[iy]; sz = a.z[iz];
  }
  float trunc = a.trunc0;
  if (kContracted) {
    const float n = sqrtf(sx * sx + sy * sy + sz * sz);
    if (n > 1.0f) trunc *= 1.0f / (2.0f - fminf(n, 1.9f));
    if (!(n < 1.0f)) {   // torch.where(mag < 1, y, 1 / (2 - mag) * (y / mag))
      const float k = 1.0f / (2.0f - n);
      sx = k * (sx / n); sy = k * (sy / n); sz = k * (sz / n);
    }
    sx = sx * a.radius + a.cx; sy = sy * a.radius + a.cy; sz = sz * a.radius + a.cz;
  }
  float tsdf = 1.0f, w = 1.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f;
  const size_t hw = (size_t)a.W * a.H;
  const float wm1 = (float)(a.W - 1), hm1 = (float)(a.H - 1);
  for (int v = 0; v < a.V; v++) {
    const float *__restrict__ M = proj + (size_t)v * 16;   // uniform address: scalar loads
    const float px = __builtin_fmaf(sz, M[8], __builtin_fmaf(sy, M[4], sx * M[0])) + M[12];
    const float py = __builtin_fmaf(sz, M[9], __builtin_fmaf(sy, M[5], sx * M[1])) + M[13];
    const float zc = __builtin_fmaf(sz, M[11], __builtin_fmaf(sy, M[7], sx * M[3])) + M[15];
    const float u = px / zc, t = py / zc;
    const bool inside = u > -1.0f && u < 1.0f && t > -1.0f && t < 1.0f && zc > 0.0f;
    if (!inside) continue;
    // grid_sample, bilinear, align_corners=True, padding_mode='border'
    const float fx = fminf(fmaxf((u + 1.0f) / 2.0f * wm1, 0.0f), wm1);
    const float fy = fminf(fmaxf((t + 1.0f) / 2.0f * hm1, 0.0f), hm1);
    const float x0f = floorf(fx), y0f = floorf(fy);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float ex = (x0f + 1.0f) - fx, ey = (y0f + 1.0f) - fy, dx = fx - x0f, dy = fy - y0f;
    const float wnw = ex * ey, wne = dx * ey, wsw = ex * dy, wse = dx * dy;
    const float *__restrict__ dm = depth + (size_t)v * hw;
    const float d = corner(dm, x0, y0, a.W, a.H) * wnw + corner(dm, x0 + 1, y0, a.W, a.H) * wne +
                    corner(dm, x0, y0 + 1, a.W, a.H) * wsw + corner(dm, x0 + 1, y0 + 1, a.W, a.H) * wse;
    const float sdf = d - zc;
    if (!(sdf > -trunc)) continue;
    const float s = fminf(fmaxf(sdf / trunc, -1.0f), 1.0f);
    const float wp = w + 1.0f;
    tsdf = (tsdf * w + s) / wp;
    if (kRgb) {
      const float *__restrict__ cm = rgb + (size_t)v * 3 * hw;
      float c[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const float *__restrict__ m = cm + (size_t)k * hw;
        c[k] = corner(m, x0, y0, a.W, a.H) * wnw + corner(m, x0 + 1, y0, a.W, a.H) * wne +
               corner(m, x0, y0 + 1, a.W, a.H) * wsw + corner(m, x0 + 1, y0 + 1, a.W, a.H) * wse;
      }
      cr = (cr * w + c[0]) / wp;
      cg = (cg * w + c[1]) / wp;
      cb = (cb * w + c[2]) / wp;
    }
    w = wp;
  }
  out_tsdf[g] = tsdf;
  if (kRgb) {
    out_rgb[g * 3 + 0] = cr; out_rgb[g * 3 + 1] = cg; out_rgb[g * 3 + 2] = cb;
  }
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" int scorp_tsdf_fuse(const ScorpTsdfViews *views, const ScorpTsdfSamples *samples, const ScorpTsdfParams *params,
                               float *out_tsdf, float *out_rgb, scorp_stream_t stream) {
  if (!views || !samples || !params || !out_tsdf) { set_error("tsdf: NULL argument"); return SCORP_ERR_INVALID; }
  if (!views->depth || !views->full_proj) { set_error("tsdf: NULL depth or full_proj"); return SCORP_ERR_INVALID; }
  if (out_rgb && !views->rgb) { set_error("tsdf: out_rgb without views->rgb"); return SCORP_ERR_INVALID; }
  if (views->num_views < 1) { set_error("tsdf: num_views < 1"); return SCORP_ERR_INVALID; }
  if (views->width < 2 || views->height < 2) { set_error("tsdf: width and height must be at least 2"); return SCORP_ERR_INVALID; }
  const uint64_t max_count = (uint64_t)0x7FFFFFFF * kTsdfThreads;
  if (samples->count < 1 || samples->count > max_count || samples->first + samples->count < samples->first) {
    set_error("tsdf: count must be in [1, (2^31 - 1) * %d]", kTsdfThreads); return SCORP_ERR_INVALID;
  }
  if (!samples->xyz) {
    if (!samples->x || !samples->y || !samples->z) { set_error("tsdf: neither points nor a lattice"); return SCORP_ERR_INVALID; }
    if (samples->nx < 1 || samples->ny < 1 || samples->nz < 1) { set_error("tsdf: empty lattice"); return SCORP_ERR_INVALID; }
    const uint64_t m = (uint64_t)samples->nx * (uint64_t)samples->ny * (uint64_t)samples->nz;
    if (samples->first + samples->count > m) { set_error("tsdf: samples past the end of the lattice"); return SCORP_ERR_INVALID; }
  }
  if (!(params->voxel_size > 0.0)) { set_error("tsdf: voxel_size must be positive"); return SCORP_ERR_INVALID; }
  if (params->contracted && !(params->radius > 0.0f)) { set_error("tsdf: radius must be positive with contracted"); return SCORP_ERR_INVALID; }
  TsdfArgs a;
  a.xyz = samples->xyz; a.x = samples->x; a.y = samples->y; a.z = samples->z;
  a.V = views->num_views; a.W = views->width; a.H = views->height;
  a.ny = samples->ny; a.nz = samples->nz;
  a.first = samples->first; a.end = samples->first + samples->count;
  a.trunc0 = (float)(5.0 * params->voxel_size);
  a.cx = params->center[0]; a.cy = params->center[1]; a.cz = params->center[2]; a.radius = params->radius;
  const unsigned blocks = (unsigned)((samples->count + kTsdfThreads - 1) / kTsdfThreads);
  hipStream_t s = (hipStream_t)stream;
  const bool c = params->contracted != 0;
  if (out_rgb) {
    if (c) tsdf_fuse_kernel<true, true><<<blocks, kTsdfThreads, 0, s>>>(a, views->full_proj, views->depth, views->rgb, out_tsdf, out_rgb);
    else tsdf_fuse_kernel<true, false><<<blocks, kTsdfThreads, 0, s>>>(a, views->full_proj, views->depth, views->rgb, out_tsdf, out_rgb);
  } else {
    if (c) tsdf_fuse_kernel<false, true><<<blocks, kTsdfThreads, 0, s>>>(a, views->full_proj, views->depth, views->rgb, out_tsdf, out_rgb);
    else tsdf_fuse_kernel<false, false><<<blocks, kTsdfThreads, 0, s>>>(a, views->full_proj, views->depth, views->rgb, out_tsdf, out_rgb);
  }
  SCORP_KERNEL_CHECK("tsdf_fuse", 0, s);
  return SCORP_OK;
}
