// depth_terms.hip — the loss terms train_3dgs.py:109-150 adds after depth_from_iter, as values and as gradients with
// respect to the rasterizer's raw outputs, without a host synchronisation:
//   depth_terms_pass1_kernel   mask counts, extrema over the estimate mask, sum of the sensor term      (pixels)
//   depth_terms_pass2_kernel   sum of the estimate term, the gradient maps g_depth_raw / g_alpha         (pixels)
//   isotropic_value_kernel     sum over the Gaussians of sum_i |s_i - mean(s)|                           (Gaussians)
//   view_terms_finalize_kernel the partial sums added in a fixed order -> out_terms4
// The estimate term normalises both depths by the extrema over ITS OWN mask (image_utils.py:87-91 applied to
// rend_depth[mask], train_3dgs.py:125-134), so its values and gradients need a first pass for counts and extrema: two
// streaming passes, ~40 MB at 1600x1200.  No float atomics: counts and extrema are integer atomics (the bit patterns of
// positive floats order like the floats), every sum is one partial per workgroup in the caller's workspace, added by one
// workgroup in a fixed order - two calls give the same bits.  Everything that is uniform over the image (the weights
// divided by counts and ranges) and the normalised depths are formed in double: the pixel's gradient then carries one
// fp32 rounding, and the sign of a difference is the sign the exact difference has.
// Contract and the degenerate cases: include/scorp_gs.h (ScorpGs3dViewTerms).
#include <math.h>

#include "common.hpp"
#include "terms_common.hpp"   // the workspace header, masks, uniforms and reductions shared with surfel_terms.hip

namespace scorp {
namespace {

struct TermsLayout {
  int blocks_px, blocks_n;
  size_t sum_sensor, sum_est, sum_iso, total;   // byte offsets of the partial sums (doubles)
  TermsLayout(int W, int H, int N) {
    blocks_px = terms_blocks((size_t)(W > 0 ? W : 0) * (size_t)(H > 0 ? H : 0));
    blocks_n = terms_blocks((size_t)(N > 0 ? N : 0));
    sum_sensor = kTermsHeaderBytes;
    sum_est = sum_sensor + sizeof(double) * blocks_px;
    sum_iso = sum_est + sizeof(double) * blocks_px;
    total = (sum_iso + sizeof(double) * blocks_n + 255) & ~(size_t)255;
  }
};

// the render()'s depth of a pixel, with render_tail_kernel's arithmetic (aux_kernels.hip)
__device__ __forceinline__ float rendered_depth(float d, float a) { return nan_to_num00(d / a); }
__global__ void __launch_bounds__(256)
depth_terms_pass1_kernel(const float *__restrict__ depth, const float *__restrict__ alpha, const float *__restrict__ sensor,
                         const float *__restrict__ est, size_t HW, TermsHeader *__restrict__ hdr, double *__restrict__ sum_sensor) {
  __shared__ double s_part[4];
  uint32_t cs = 0, ce = 0, inv_rmin = 0, rmax = 0, inv_pmin = 0, pmax = 0;
  double sum = 0.0;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += stride) {
    const float r = rendered_depth(depth[i], alpha[i]);
    if (sensor) {
      const float s = sensor[i];
      if (in_sensor_mask(r, s)) { cs++; sum += fabs((double)r - (double)s); }
    }
    if (est) {
      const float e = est[i];
      if (in_est_mask(r, e)) {   // both positive: their bit patterns order like the values
        ce++;
        const uint32_t rb = __float_as_uint(r), eb = __float_as_uint(e);
        inv_rmin = max(inv_rmin, ~rb); rmax = max(rmax, rb);
        inv_pmin = max(inv_pmin, ~eb); pmax = max(pmax, eb);
      }
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
  const double total = block_sum(sum, s_part);
  if (threadIdx.x == 0) sum_sensor[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256)
depth_terms_pass2_kernel(const float *__restrict__ depth, const float *__restrict__ alpha, const float *__restrict__ sensor,
                         const float *__restrict__ est, size_t HW, float w_sensor, float w_est,
                         const TermsHeader *__restrict__ hdr, double *__restrict__ sum_est, float *__restrict__ g_depth,
                         float *__restrict__ g_alpha) {
  __shared__ double s_part[4];
  const TermsUniform u = terms_uniform(hdr, w_sensor, w_est);
  double sum = 0.0;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < HW; i += stride) {
    const float d = depth[i], a = alpha[i], q = d / a;
    const float r = nan_to_num00(q);
    double g64 = 0.0;
    if (sensor) {
      const float s = sensor[i];
      if (in_sensor_mask(r, s)) g64 += r > s ? u.ks : r < s ? -u.ks : 0.0;
    }
    if (est && u.est_ok) {
      const float e = est[i];
      if (in_est_mask(r, e)) {
        const double diff = ((double)r - u.rmin) * u.inv_rrange - ((double)e - u.pmin) * u.inv_prange;
        sum += fabs(diff);
        g64 += diff > 0.0 ? u.ke : diff < 0.0 ? -u.ke : 0.0;
      }
    }
    // through nan_to_num(depth / alpha): render_tail_backward_kernel's expressions (aux_kernels.hip)
    const bool pass = a != 0.0f && q == q && fabsf(q) != __builtin_inff();
    const float g = pass ? (float)g64 : 0.0f;
    g_depth[i] = pass ? g / a : 0.0f;
    g_alpha[i] = pass ? -g * d / (a * a) : 0.0f;
  }
  const double total = block_sum(sum, s_part);
  if (threadIdx.x == 0) sum_est[blockIdx.x] = total;
}

// sum_n sum_i |s_ni - mean_i s_ni| of the scales as the model activates them (raw bit 1: exp), gs3dgs/utils/loss_utils.py:75-85
__global__ void __launch_bounds__(256)
isotropic_value_kernel(const float *__restrict__ scales, int N, int raw, double *__restrict__ sum_iso) {
  __shared__ double s_part[4];
  double sum = 0.0;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)N; i += stride) {
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { const float v = scales[3 * i + k]; s[k] = (raw & 2) ? expf(v) : v; }
    const double m = (s[0] + s[1] + s[2]) / 3.0;
    sum += fabs(s[0] - m) + fabs(s[1] - m) + fabs(s[2] - m);
  }
  const double total = block_sum(sum, s_part);
  if (threadIdx.x == 0) sum_iso[blockIdx.x] = total;
}

// One workgroup: thread t adds partials t, t + 256, ... in order, then the workgroup's fixed tree.  out_terms4 =
// {w_sensor Ls + w_est Le + lambda_iso Liso, Ls, Le, Liso}; a term that was not asked for is 0, a degenerate one NaN.
__global__ void __launch_bounds__(256)
view_terms_finalize_kernel(const TermsHeader *__restrict__ hdr, const double *__restrict__ sum_sensor,
                           const double *__restrict__ sum_est, const double *__restrict__ sum_iso, int blocks_px, int blocks_n,
                           int has_sensor, int has_est, int N, float w_sensor, float w_est, float lambda_iso,
                           float *__restrict__ out_terms4) {
  __shared__ double s_part[4];
  double ps = 0.0, pe = 0.0, pi = 0.0;
  if (has_sensor) for (int b = threadIdx.x; b < blocks_px; b += 256) ps += sum_sensor[b];
  if (has_est) for (int b = threadIdx.x; b < blocks_px; b += 256) pe += sum_est[b];
  if (sum_iso) for (int b = threadIdx.x; b < blocks_n; b += 256) pi += sum_iso[b];
  ps = block_sum(ps, s_part); __syncthreads();
  pe = block_sum(pe, s_part); __syncthreads();
  pi = block_sum(pi, s_part);
  if (threadIdx.x != 0) return;
  const double qnan = __builtin_nan("");
  double Ls = 0.0, Le = 0.0, Li = 0.0, total = 0.0;
  if (has_sensor) { Ls = hdr->count_sensor > 0 ? ps / (double)hdr->count_sensor : qnan; total += (double)w_sensor * Ls; }
  if (has_est) {
    const TermsUniform u = terms_uniform(hdr, w_sensor, w_est);
    Le = u.est_ok ? pe / (double)hdr->count_est : qnan;
    total += (double)w_est * Le;
  }
  if (sum_iso) { Li = pi / (3.0 * (double)N); total += (double)lambda_iso * Li; }   // (N > 0: the caller's condition)
  out_terms4[0] = (float)total; out_terms4[1] = (float)Ls; out_terms4[2] = (float)Le; out_terms4[3] = (float)Li;
}

}  // namespace

// The launches of one set of terms; the arguments were checked by the caller.  `scales` NULL: no isotropic value.
int view_terms_impl(int W, int H, const float *depth_raw, const float *alpha, const float *sensor, const float *est,
                    float w_sensor, float w_est, const float *scales, int N, int raw, float lambda_iso, float *out_terms4,
                    float *g_depth_raw, float *g_alpha, void *workspace, hipStream_t stream) {
  const TermsLayout T(W, H, N);
  char *ws = (char *)workspace;
  TermsHeader *hdr = (TermsHeader *)ws;
  double *sum_sensor = (double *)(ws + T.sum_sensor), *sum_est = (double *)(ws + T.sum_est), *sum_iso = (double *)(ws + T.sum_iso);
  const size_t HW = (size_t)W * (size_t)H;
  const bool depth_terms = (sensor || est) && HW > 0;
  SCORP_HIP_CHECK(hipMemsetAsync(hdr, 0, kTermsHeaderBytes, stream));
  if (depth_terms) {
    depth_terms_pass1_kernel<<<T.blocks_px, 256, 0, stream>>>(depth_raw, alpha, sensor, est, HW, hdr, sum_sensor);
    SCORP_KERNEL_CHECK("depth_terms_pass1", 0, stream);
    depth_terms_pass2_kernel<<<T.blocks_px, 256, 0, stream>>>(depth_raw, alpha, sensor, est, HW, w_sensor, w_est, hdr, sum_est,
                                                              g_depth_raw, g_alpha);
    SCORP_KERNEL_CHECK("depth_terms_pass2", 0, stream);
  }
  const bool iso = scales != nullptr && N > 0;
  if (iso) {
    isotropic_value_kernel<<<T.blocks_n, 256, 0, stream>>>(scales, N, raw, sum_iso);
    SCORP_KERNEL_CHECK("isotropic_value", 0, stream);
  }
  view_terms_finalize_kernel<<<1, 256, 0, stream>>>(hdr, sum_sensor, sum_est, iso ? sum_iso : nullptr,
                                                    depth_terms ? T.blocks_px : 0, iso ? T.blocks_n : 0, sensor != nullptr,
                                                    est != nullptr, N, w_sensor, w_est, lambda_iso, out_terms4);
  SCORP_KERNEL_CHECK("view_terms_finalize", 0, stream);
  return SCORP_OK;
}

}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_gs3d_view_terms_workspace_bytes(int32_t W, int32_t H, int32_t N) { return TermsLayout(W, H, N).total; }

extern "C" int scorp_gs3d_depth_terms(int32_t W, int32_t H, const float *depth_raw, const float *alpha, const float *depth_sensor,
                                      const float *depth_est, float lambda_depth_sensor, float weight_depth_est,
                                      float *out_terms4, float *grad_depth_raw, float *grad_alpha, void *workspace,
                                      size_t workspace_bytes, scorp_stream_t stream) {
  if (W <= 0 || H <= 0) { set_error("scorp_gs3d_depth_terms: image %d x %d", W, H); return SCORP_ERR_INVALID; }
  if (!depth_raw || !alpha || !out_terms4 || !grad_depth_raw || !grad_alpha) {
    set_error("scorp_gs3d_depth_terms: depth_raw, alpha, out_terms4, grad_depth_raw or grad_alpha is NULL");
    return SCORP_ERR_INVALID;
  }
  if (!depth_sensor && !depth_est) { set_error("scorp_gs3d_depth_terms: neither depth_sensor nor depth_est"); return SCORP_ERR_INVALID; }
  const size_t need = TermsLayout(W, H, 0).total;
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15)) {
    set_error("scorp_gs3d_depth_terms: workspace NULL, misaligned or too small (%zu < %zu)", workspace_bytes, need);
    return SCORP_ERR_INVALID;
  }
  return view_terms_impl(W, H, depth_raw, alpha, depth_sensor, depth_est, lambda_depth_sensor, weight_depth_est, nullptr, 0, 0,
                         0.0f, out_terms4, grad_depth_raw, grad_alpha, workspace, (hipStream_t)stream);
}
