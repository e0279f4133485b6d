// gs2d_maps.hpp — what the kernels over the 2DGS per-pixel maps share (gs2d_maps.hip: the maps' forward / backward and the
// regularisers; surfel_terms.hip: the late iterations' loss terms): the camera arguments, the surface depth of a pixel,
// the back-projected points and the frame of a pseudo normal.  See gs2d_maps.hip for the formulation.
#pragma once
#include "common.hpp"

namespace scorp {
namespace {
constexpr float kNormEps = 1e-12f;  // torch.nn.functional.normalize default eps

struct MapsDev {
  int W, H;
  float depth_ratio;
  const float *view;    // world_view_transform, 4x4 row-major as torch stores it (device)
  const float *rays_o;  // [3] (device)
};
struct MapsArgs {
  int W, H;
  float depth_ratio;
  float V[9];   // world_view_transform[:3,:3]
  float ro[3];
  __device__ explicit MapsArgs(const MapsDev &d) : W(d.W), H(d.H), depth_ratio(d.depth_ratio) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
#pragma unroll
      for (int i = 0; i < 3; i++) V[j * 3 + i] = d.view[j * 4 + i];
      ro[j] = d.rays_o[j];
    }
  }
};

__device__ __forceinline__ bool passes_grad(float x) { return x == x && fabsf(x) != __builtin_inff(); }

__device__ __forceinline__ float surf_depth_of(const float *__restrict__ allmap, size_t HW, size_t p, float r) {
  const float e = nan_to_num00(allmap[p] / allmap[HW + p]);
  const float m = nan_to_num00(allmap[5 * HW + p]);
  return e * (1.0f - r) + r * m;
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

__device__ __forceinline__ V3 point_of(float d, const float *__restrict__ rays_d, size_t p, const float *ro) {
#pragma clang fp contract(off)
  return {d * rays_d[3 * p] + ro[0], d * rays_d[3 * p + 1] + ro[1], d * rays_d[3 * p + 2] + ro[2]};
}

// Where the backward takes its upstream gradients from.  kReg = false: the five gradient maps of an arbitrary loss
// (scorp_gs2d_maps_backward).  kReg = true: the two regularisers of train_2dgs.py:142-150 fused in —
// normal_loss = lambda_n * mean(1 - rend_normal . surf_normal), dist_loss = lambda_d * mean(render_dist) — whose
// gradient maps are scaled copies of the OTHER map (d/d rend_normal = -k surf_normal, d/d surf_normal = -k rend_normal,
// d/d dist = k_d) and are re-derived from allmap on the fly; the surface depth is recomputed instead of stored.
struct MapsGrads {
  const float *sd, *g_alpha, *g_rn, *g_dist, *g_sd, *g_sn;   // kReg = false
  float kn, kd;                                               // kReg = true: lambda_n * g0 / HW, lambda_d * g1 / HW
};

template <bool kReg>
__device__ __forceinline__ float depth_at(const MapsArgs &a, const MapsGrads &G, const float *__restrict__ allmap, size_t HW, size_t q) {
  return kReg ? surf_depth_of(allmap, HW, q, a.depth_ratio) : G.sd[q];
}

// world-space rendered normal at pixel q (what render() returns as render_normal)
__device__ __forceinline__ V3 world_normal(const MapsArgs &a, const float *__restrict__ allmap, size_t HW, size_t q) {
  const float n0 = allmap[2 * HW + q], n1 = allmap[3 * HW + q], n2 = allmap[4 * HW + q];
  return {n0 * a.V[0] + n1 * a.V[1] + n2 * a.V[2], n0 * a.V[3] + n1 * a.V[4] + n2 * a.V[5], n0 * a.V[6] + n1 * a.V[7] + n2 * a.V[8]};
}

// the two difference vectors of the normal centred at pixel c (must be interior), their cross product and its length
template <bool kReg>
__device__ __forceinline__ void centre_frame(const MapsArgs &a, const MapsGrads &G, const float *__restrict__ rays_d,
                                             const float *__restrict__ allmap, size_t HW, size_t c, V3 &dv, V3 &dh, V3 &cr,
                                             float &len) {
  const size_t pu = c - a.W, pd = c + a.W, pl = c - 1, pr = c + 1;
  dv = point_of(depth_at<kReg>(a, G, allmap, HW, pd), rays_d, pd, a.ro) - point_of(depth_at<kReg>(a, G, allmap, HW, pu), rays_d, pu, a.ro);
  dh = point_of(depth_at<kReg>(a, G, allmap, HW, pr), rays_d, pr, a.ro) - point_of(depth_at<kReg>(a, G, allmap, HW, pl), rays_d, pl, a.ro);
  cr = cross3(dv, dh);
  len = sqrtf(dot3(cr, cr));
}

inline int fill_args(MapsDev &a, int W, int H, const float *viewmatrix, const float *rays_o, float depth_ratio) {
  if (W <= 0 || H <= 0) { set_error("bad image size %dx%d", W, H); return SCORP_ERR_INVALID; }
  if (!viewmatrix || !rays_o) { set_error("viewmatrix / rays_o is NULL"); return SCORP_ERR_INVALID; }
  a.W = W; a.H = H; a.depth_ratio = depth_ratio; a.view = viewmatrix; a.rays_o = rays_o;
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp
