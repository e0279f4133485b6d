// terms_common.hpp — what the two sets of late-iteration loss-term kernels share (depth_terms.hip for 3DGS,
// surfel_terms.hip for 2DGS): the header of their workspace, the masks of the two depth terms, the uniforms the second
// pass derives from the first, and the fixed-order reductions.  Contract: include/scorp_gs.h (ScorpGs3dViewTerms).
#pragma once
#include "common.hpp"

namespace scorp {
namespace {

constexpr int kTermsHeaderBytes = 64;
constexpr int kTermsMaxBlocks = 1024;

// The head of the workspace, cleared before pass 1.  The minima are kept as ~bits under atomicMax, so that zero is the
// neutral element of all six words.
struct TermsHeader {
  uint32_t count_sensor, count_est, inv_rmin, rmax, inv_pmin, pmax;
};

inline int terms_blocks(size_t n) {   // 1024 elements per workgroup and round, at most kTermsMaxBlocks workgroups
  const size_t b = (n + 1023) / 1024;
  return (int)(b < 1 ? 1 : b > (size_t)kTermsMaxBlocks ? (size_t)kTermsMaxBlocks : b);
}

__device__ __forceinline__ bool in_sensor_mask(float r, float s) {
  return s > SCORP_DEPTH_SENSOR_MIN && s < SCORP_DEPTH_SENSOR_MAX && r > 0.0f;
}
__device__ __forceinline__ bool in_est_mask(float r, float e) { return r > 0.0f && e > 0.0f; }

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
// the workgroup's sum in thread 0 (four waves; the order is fixed)
__device__ __forceinline__ double block_sum(double x, double *s_part) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = x;
  __syncthreads();
  return (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}
__device__ __forceinline__ uint32_t wave_max(uint32_t x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = max(x, (uint32_t)__shfl_xor((int)x, off, 64));
  return x;
}
__device__ __forceinline__ uint32_t wave_add(uint32_t x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += (uint32_t)__shfl_xor((int)x, off, 64);
  return x;
}

// What pass 2 and the finalize kernel derive from the header: the terms' per-pixel gradient magnitudes (zero for a
// degenerate term) and the estimate term's normalisation.
struct TermsUniform {
  double ks, ke, rmin, inv_rrange, pmin, inv_prange;
  bool est_ok;
};
__device__ __forceinline__ TermsUniform terms_uniform(const TermsHeader *hdr, float w_sensor, float w_est) {
  TermsUniform u;
  const uint32_t cs = hdr->count_sensor, ce = hdr->count_est;
  const double rmin = __uint_as_float(~hdr->inv_rmin), rmax = __uint_as_float(hdr->rmax);
  const double pmin = __uint_as_float(~hdr->inv_pmin), pmax = __uint_as_float(hdr->pmax);
  u.est_ok = ce > 0 && rmax > rmin && pmax > pmin;
  u.ks = cs > 0 ? (double)w_sensor / (double)cs : 0.0;
  u.rmin = u.est_ok ? rmin : 0.0; u.pmin = u.est_ok ? pmin : 0.0;
  u.inv_rrange = u.est_ok ? 1.0 / (rmax - rmin) : 0.0;
  u.inv_prange = u.est_ok ? 1.0 / (pmax - pmin) : 0.0;
  u.ke = u.est_ok ? (double)w_est / ((rmax - rmin) * (double)ce) : 0.0;
  return u;
}

}  // namespace
}  // namespace scorp
