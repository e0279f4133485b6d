// surfel_terms.hip — the loss terms train_2dgs.py:100-139 adds after depth_from_iter, on the 2DGS allmap, as values and as
// the gradient maps the maps' backward (gs2d_maps.hip, maps_backward_terms_kernel) folds into its one pass over grad_allmap:
//   surfel_terms_pass1_kernel     the surface depth d (gs2d_maps.hpp, surf_depth_of) -> out_depth; mask counts, extrema over
//                                 the estimate mask, the sensor sum; with the depth-normal weight: the normal of the ESTIMATED
//                                 depth map (point_utils.py:9-37), the sums of 1 - surf_normal . pred_normal and
//                                 1 - rend_normal . pred_normal, and g_normal = -(w_n / HW) pred_normal                (pixels, 64 x 4 tiles)
//   surfel_terms_pass2_kernel     the estimate sum, g_depth = d loss / d d of the two depth terms                      (pixels)
//   isotropic2_value_kernel       sum over the surfels of |s_0 - m| + |s_1 - m|                                         (surfels)
//   surfel_terms_finalize_kernel  the partial sums added in a fixed order -> out_terms6
// The depth terms are those of depth_terms.hip with d in place of r: same masks, constants and double-precision uniforms
// (terms_common.hpp).  pred_normal is computed ONCE per view, in pass 1, and kept as the already weighted gradient map
// g_normal: it is the upstream gradient of both surf_normal and render_normal, so the backward reads three floats per
// normal centre instead of staging a second tile of back-projected points in LDS, which would cost it a workgroup per CU.
// No float atomics: counts and extrema are integer atomics, every sum is one partial per workgroup, added by one workgroup
// in a fixed order - two calls give the same bits.  Contract and the degenerate cases: include/scorp_gs.h (ScorpGs2dViewTerms).
#include <math.h>

#include "common.hpp"
#include "gs2d_maps.hpp"
#include "terms_common.hpp"

namespace scorp {
namespace {

inline int tile_blocks(int W, int H) { return ((W + 63) / 64) * ((H + 3) / 4); }

struct SurfelTermsLayout {
  int blocks_tile, blocks_px, blocks_n;
  size_t sum_sensor, sum_dn, sum_rn, sum_est, sum_iso, total;   // byte offsets of the partial sums (doubles)
  SurfelTermsLayout(int W, int H, int N) {
    W = W > 0 ? W : 0; H = H > 0 ? H : 0;
    blocks_tile = tile_blocks(W, H) < 1 ? 1 : tile_blocks(W, H) > kTermsMaxBlocks ? kTermsMaxBlocks : tile_blocks(W, H);
    blocks_px = terms_blocks((size_t)W * (size_t)H);
    blocks_n = terms_blocks((size_t)(N > 0 ? N : 0));
    sum_sensor = kTermsHeaderBytes;
    sum_dn = sum_sensor + sizeof(double) * blocks_tile;
    sum_rn = sum_dn + sizeof(double) * blocks_tile;
    sum_est = sum_rn + sizeof(double) * blocks_tile;
    sum_iso = sum_est + sizeof(double) * blocks_px;
    total = (sum_iso + sizeof(double) * blocks_n + 255) & ~(size_t)255;
  }
};

// kNormal: the depth-normal terms too (needs est).  One thread per pixel of a 64 x 4 tile, as the regularisers' forward; a
// workgroup takes tiles b, b + gridDim.x, ... (at most kTermsMaxBlocks workgroups), so that the integer atomics on the one
// header line are a few thousand per view and not one set per wave of the image (they serialise: 2 ms at 1600 x 1200).
template <bool kNormal>
__global__ void __launch_bounds__(256)
surfel_terms_pass1_kernel(MapsDev dev, const float *__restrict__ allmap, const float *__restrict__ rays_d,
                          const float *__restrict__ sensor, const float *__restrict__ est, float kn, TermsHeader *__restrict__ hdr,
                          double *__restrict__ sum_sensor, double *__restrict__ sum_dn, double *__restrict__ sum_rn,
                          float *__restrict__ out_depth, float *__restrict__ g_normal) {
  const MapsArgs a(dev);
  __shared__ double s_part[4];
  const int tiles_x = (a.W + 63) / 64, tiles = tiles_x * ((a.H + 3) / 4);
  uint32_t cs = 0, ce = 0, inv_rmin = 0, rmax = 0, inv_pmin = 0, pmax = 0;
  double ssum = 0.0, tdn = 0.0, trn = 0.0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int x = (t % tiles_x) * 64 + (threadIdx.x & 63), y = (t / tiles_x) * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) continue;
    const size_t HW = (size_t)a.W * a.H, p = (size_t)y * a.W + x;
    const float d = surf_depth_of(allmap, HW, p, a.depth_ratio);
    out_depth[p] = d;
    if (sensor) {
      const float s = sensor[p];
      if (in_sensor_mask(d, s)) { cs++; ssum += fabs((double)d - (double)s); }
    }
    if (est) {
      const float e = est[p];
      if (in_est_mask(d, e)) {   // both positive: their bit patterns order like the values
        ce++;
        const uint32_t rb = __float_as_uint(d), eb = __float_as_uint(e);
        inv_rmin = max(inv_rmin, ~rb); rmax = max(rmax, rb); inv_pmin = max(inv_pmin, ~eb); pmax = max(pmax, eb);
      }
    }
    if constexpr (kNormal) {
      V3 pn = {0.0f, 0.0f, 0.0f};
      float dot_sn = 0.0f, dot_rn = 0.0f;
      if (x >= 1 && y >= 1 && x < a.W - 1 && y < a.H - 1) {
        const size_t pu = p - a.W, pd = p + a.W, pl = p - 1, pr = p + 1;
        const V3 ev = point_of(est[pd], rays_d, pd, a.ro) - point_of(est[pu], rays_d, pu, a.ro);
        const V3 eh = point_of(est[pr], rays_d, pr, a.ro) - point_of(est[pl], rays_d, pl, a.ro);
        const V3 ec = cross3(ev, eh);
        const float einv = 1.0f / fmaxf(sqrtf(dot3(ec, ec)), kNormEps);
        pn = {ec.x * einv, ec.y * einv, ec.z * einv};
        MapsGrads none = {};
        V3 dv, dh, cr;
        float len;
        centre_frame<true>(a, none, rays_d, allmap, HW, p, dv, dh, cr, len);
        dot_sn = dot3(pn, cr) * (allmap[HW + p] / fmaxf(len, kNormEps));
        dot_rn = dot3(pn, world_normal(a, allmap, HW, p));
      }
      tdn += 1.0 - (double)dot_sn; trn += 1.0 - (double)dot_rn;
      g_normal[p] = -kn * pn.x; g_normal[HW + p] = -kn * pn.y; g_normal[2 * HW + p] = -kn * pn.z;
    }
  }
  cs = wave_add(cs); ce = wave_add(ce);
  inv_rmin = wave_max(inv_rmin); rmax = wave_max(rmax); inv_pmin = wave_max(inv_pmin); pmax = wave_max(pmax);
  if ((threadIdx.x & 63) == 0) {
    if (cs) atomicAdd(&hdr->count_sensor, cs);
    if (ce) {
      atomicAdd(&hdr->count_est, ce);
      atomicMax(&hdr->inv_rmin, inv_rmin); atomicMax(&hdr->rmax, rmax);
      atomicMax(&hdr->inv_pmin, inv_pmin); atomicMax(&hdr->pmax, pmax);
    }
  }
  const int b = blockIdx.x;
  if (sensor) {
    const double ts = block_sum(ssum, s_part);
    if (threadIdx.x == 0) sum_sensor[b] = ts;
  }
  if constexpr (kNormal) {
    __syncthreads();
    const double t1 = block_sum(tdn, s_part);
    __syncthreads();
    const double t2 = block_sum(trn, s_part);
    if (threadIdx.x == 0) { sum_dn[b] = t1; sum_rn[b] = t2; }
  }
}

__global__ void __launch_bounds__(256)
surfel_terms_pass2_kernel(const float *__restrict__ depth, const float *__restrict__ sensor, const float *__restrict__ est,
                          size_t HW, float w_sensor, float w_est, const TermsHeader *__restrict__ hdr,
                          double *__restrict__ sum_est, float *__restrict__ g_depth) {
  __shared__ double s_part[4];
  const TermsUniform u = terms_uniform(hdr, w_sensor, w_est);
  double sum = 0.0;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += stride) {
    const float d = depth[i];
    double g64 = 0.0;
    if (sensor) {
      const float s = sensor[i];
      if (in_sensor_mask(d, s)) g64 += d > s ? u.ks : d < s ? -u.ks : 0.0;
    }
    if (est && u.est_ok) {
      const float e = est[i];
      if (in_est_mask(d, e)) {
        const double diff = ((double)d - u.rmin) * u.inv_rrange - ((double)e - u.pmin) * u.inv_prange;
        sum += fabs(diff);
        g64 += diff > 0.0 ? u.ke : diff < 0.0 ? -u.ke : 0.0;
      }
    }
    g_depth[i] = (float)g64;   // (through the depth_ratio mix and nan_to_num: the maps' backward)
  }
  const double total = block_sum(sum, s_part);
  if (threadIdx.x == 0) sum_est[blockIdx.x] = total;
}

// sum_n |s_n0 - m_n| + |s_n1 - m_n| of the [N,2] scales as the model activates them (raw bit 1: exp)
__global__ void __launch_bounds__(256)
isotropic2_value_kernel(const float *__restrict__ scales, int N, int raw, double *__restrict__ sum_iso) {
  __shared__ double s_part[4];
  double sum = 0.0;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)N; i += stride) {
    const float2 v = reinterpret_cast<const float2 *>(scales)[i];
    const double s0 = (raw & 2) ? expf(v.x) : v.x, s1 = (raw & 2) ? expf(v.y) : v.y;
    const double m = (s0 + s1) / 2.0;
    sum += fabs(s0 - m) + fabs(s1 - m);
  }
  const double total = block_sum(sum, s_part);
  if (threadIdx.x == 0) sum_iso[blockIdx.x] = total;
}

struct SurfelTermsWeights { float sensor, est, normal, iso; };

// One workgroup: thread t adds partials t, t + 256, ... in order, then the workgroup's fixed tree.  out_terms6 =
// {w_s Ls + w_e Le + w_n (Ldn + Lrn) + lambda_iso Liso, Ls, Le, Ldn, Lrn, Liso}; a term that was not asked for is 0, a
// degenerate depth term NaN.
__global__ void __launch_bounds__(256)
surfel_terms_finalize_kernel(const TermsHeader *__restrict__ hdr, const double *__restrict__ sum_sensor,
                             const double *__restrict__ sum_dn, const double *__restrict__ sum_rn,
                             const double *__restrict__ sum_est, const double *__restrict__ sum_iso, int blocks_tile,
                             int blocks_px, int blocks_n, int has_sensor, int has_est, int has_normal, double HW, int N,
                             SurfelTermsWeights w, float *__restrict__ out_terms6) {
  __shared__ double s_part[4];
  double ps = 0.0, pe = 0.0, pdn = 0.0, prn = 0.0, pi = 0.0;
  if (has_sensor) for (int b = threadIdx.x; b < blocks_tile; b += 256) ps += sum_sensor[b];
  if (has_normal) for (int b = threadIdx.x; b < blocks_tile; b += 256) { pdn += sum_dn[b]; prn += sum_rn[b]; }
  if (has_est) for (int b = threadIdx.x; b < blocks_px; b += 256) pe += sum_est[b];
  if (sum_iso) for (int b = threadIdx.x; b < blocks_n; b += 256) pi += sum_iso[b];
  ps = block_sum(ps, s_part); __syncthreads();
  pe = block_sum(pe, s_part); __syncthreads();
  pdn = block_sum(pdn, s_part); __syncthreads();
  prn = block_sum(prn, s_part); __syncthreads();
  pi = block_sum(pi, s_part);
  if (threadIdx.x != 0) return;
  const double qnan = __builtin_nan("");
  double Ls = 0.0, Le = 0.0, Ldn = 0.0, Lrn = 0.0, Li = 0.0, total = 0.0;
  if (has_sensor) { Ls = hdr->count_sensor > 0 ? ps / (double)hdr->count_sensor : qnan; total += (double)w.sensor * Ls; }
  if (has_est) {
    const TermsUniform u = terms_uniform(hdr, w.sensor, w.est);
    Le = u.est_ok ? pe / (double)hdr->count_est : qnan;
    total += (double)w.est * Le;
  }
  if (has_normal) { Ldn = pdn / HW; Lrn = prn / HW; total += (double)w.normal * (Ldn + Lrn); }
  if (sum_iso) { Li = pi / (2.0 * (double)N); total += (double)w.iso * Li; }   // (N > 0: the caller's condition)
  out_terms6[0] = (float)total; out_terms6[1] = (float)Ls; out_terms6[2] = (float)Le;
  out_terms6[3] = (float)Ldn; out_terms6[4] = (float)Lrn; out_terms6[5] = (float)Li;
}

}  // namespace

// The launches of one set of terms; the arguments were checked by the caller.  `scales` NULL: no isotropic value.
int surfel_terms_impl(int W, int H, const float *allmap, const float *viewmatrix, const float *rays_d, const float *rays_o,
                      float depth_ratio, const float *sensor, const float *est, float w_sensor, float w_est, float w_normal,
                      const float *scales, int N, int raw, float lambda_iso, float *out_terms6, float *out_depth, float *g_depth,
                      float *g_normal, void *workspace, hipStream_t stream) {
  const SurfelTermsLayout T(W, H, N);
  char *ws = (char *)workspace;
  TermsHeader *hdr = (TermsHeader *)ws;
  double *sum_sensor = (double *)(ws + T.sum_sensor), *sum_dn = (double *)(ws + T.sum_dn), *sum_rn = (double *)(ws + T.sum_rn);
  double *sum_est = (double *)(ws + T.sum_est), *sum_iso = (double *)(ws + T.sum_iso);
  const size_t HW = (size_t)W * (size_t)H;
  const bool depth_terms = (sensor || est) && HW > 0;
  const bool normal = depth_terms && est && w_normal != 0.0f;
  SCORP_HIP_CHECK(hipMemsetAsync(hdr, 0, kTermsHeaderBytes, stream));
  if (depth_terms) {
    MapsDev a;
    if (int e = fill_args(a, W, H, viewmatrix, rays_o, depth_ratio)) return e;
    const dim3 grid(T.blocks_tile);
    const float kn = (float)((double)w_normal / (double)HW);
    if (normal)
      surfel_terms_pass1_kernel<true><<<grid, 256, 0, stream>>>(a, allmap, rays_d, sensor, est, kn, hdr, sum_sensor, sum_dn, sum_rn,
                                                               out_depth, g_normal);
    else
      surfel_terms_pass1_kernel<false><<<grid, 256, 0, stream>>>(a, allmap, rays_d, sensor, est, 0.0f, hdr, sum_sensor, sum_dn,
                                                                sum_rn, out_depth, nullptr);
    SCORP_KERNEL_CHECK("surfel_terms_pass1", 0, stream);
    surfel_terms_pass2_kernel<<<T.blocks_px, 256, 0, stream>>>(out_depth, sensor, est, HW, w_sensor, w_est, hdr, sum_est, g_depth);
    SCORP_KERNEL_CHECK("surfel_terms_pass2", 0, stream);
  }
  const bool iso = scales != nullptr && N > 0;
  if (iso) {
    isotropic2_value_kernel<<<T.blocks_n, 256, 0, stream>>>(scales, N, raw, sum_iso);
    SCORP_KERNEL_CHECK("isotropic2_value", 0, stream);
  }
  const SurfelTermsWeights w = {w_sensor, w_est, w_normal, lambda_iso};
  surfel_terms_finalize_kernel<<<1, 256, 0, stream>>>(hdr, sum_sensor, sum_dn, sum_rn, sum_est, iso ? sum_iso : nullptr,
                                                      depth_terms ? T.blocks_tile : 0, depth_terms ? T.blocks_px : 0,
                                                      iso ? T.blocks_n : 0, depth_terms && sensor != nullptr,
                                                      depth_terms && est != nullptr, normal, (double)HW, N, w, out_terms6);
  SCORP_KERNEL_CHECK("surfel_terms_finalize", 0, stream);
  return SCORP_OK;
}

}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_gs2d_view_terms_workspace_bytes(int32_t W, int32_t H, int32_t N) { return SurfelTermsLayout(W, H, N).total; }

extern "C" int scorp_gs2d_surfel_terms(int32_t W, int32_t H, const float *allmap, const float *viewmatrix, const float *rays_d,
                                       const float *rays_o, float depth_ratio, const float *depth_sensor, const float *depth_est,
                                       float lambda_depth_sensor, float weight_depth_est, float weight_depth_normal,
                                       float *out_terms6, float *out_depth, float *grad_depth, float *grad_normal,
                                       float *grad_allmap, void *workspace, size_t workspace_bytes, scorp_stream_t stream) {
  if (W <= 0 || H <= 0) { set_error("scorp_gs2d_surfel_terms: image %d x %d", W, H); return SCORP_ERR_INVALID; }
  if (!allmap || !viewmatrix || !rays_d || !rays_o || !out_terms6 || !out_depth || !grad_depth || !grad_allmap) {
    set_error("scorp_gs2d_surfel_terms: allmap, viewmatrix, rays_d, rays_o, out_terms6, out_depth, grad_depth or grad_allmap is NULL");
    return SCORP_ERR_INVALID;
  }
  if (!depth_sensor && !depth_est) { set_error("scorp_gs2d_surfel_terms: neither depth_sensor nor depth_est"); return SCORP_ERR_INVALID; }
  if (lambda_depth_sensor != 0.0f && !depth_sensor) { set_error("scorp_gs2d_surfel_terms: lambda_depth_sensor without depth_sensor"); return SCORP_ERR_INVALID; }
  if ((weight_depth_est != 0.0f || weight_depth_normal != 0.0f) && !depth_est) {
    set_error("scorp_gs2d_surfel_terms: weight_depth_est / weight_depth_normal without depth_est"); return SCORP_ERR_INVALID;
  }
  if (weight_depth_normal != 0.0f && !grad_normal) { set_error("scorp_gs2d_surfel_terms: weight_depth_normal needs grad_normal"); return SCORP_ERR_INVALID; }
  const size_t need = SurfelTermsLayout(W, H, 0).total;
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15)) {
    set_error("scorp_gs2d_surfel_terms: workspace NULL, misaligned or too small (%zu < %zu)", workspace_bytes, need);
    return SCORP_ERR_INVALID;
  }
  hipStream_t hs = (hipStream_t)stream;
  if (int e = surfel_terms_impl(W, H, allmap, viewmatrix, rays_d, rays_o, depth_ratio, depth_sensor, depth_est, lambda_depth_sensor,
                                weight_depth_est, weight_depth_normal, nullptr, 0, 0, 0.0f, out_terms6, out_depth, grad_depth,
                                grad_normal, workspace, hs)) return e;
  const float *gn = weight_depth_normal != 0.0f ? grad_normal : nullptr;
  return maps_backward_terms_impl(W, H, allmap, viewmatrix, rays_d, rays_o, depth_ratio, 0.0f, 0.0f, grad_depth, gn, gn, grad_allmap, hs);
}
