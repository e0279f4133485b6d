// surfel.hpp — the 2DGS surfel record and the per-pixel ray-surfel intersection, shared by the blend kernels of
// gs2d_forward.hip / gs2d_backward.hip and the mask vote (mask_vote.hip): every kernel that replays a 2-D render evaluates
// alpha with these functions, so all of them see the forward's alpha bit for bit.  Also what more than one of the three
// surfel files (gs2d_pergaussian.hip, gs2d_forward.hip, gs2d_backward.hip) needs: the constants, the accumulator row,
// the exact footprint test and the kind's entry of the shared host pipeline.
#pragma once
#include "common.hpp"

namespace scorp {

constexpr float kFilterInvSq = 2.0f;
constexpr float kFarZ = 100.0f;
constexpr float kCutoff = 3.0f;
constexpr float kFilterSize = 0.707106f;
constexpr float kExtentFloor = 0.0001f;
constexpr int kAcc2Stride = 20;  // d/d(pa, pb, pc)[9], d/dD, d/dTw.z, gxy[2], gnormal[3], gopacity, grgb[3]

constexpr GsKind kGs2d = {true, true, false, kAcc2Stride, kKPreprocess2d, kKBlendBackward2d, kKPreprocessBackward2d,
                          launch_reduce_pair_rows<kAcc2Stride, kAcc2Stride, 32>};

struct alignas(16) Surfel {  // 96 bytes, gathered as six 16-byte loads
  float4 r0;  // Tu.x Tu.y Tu.z Tv.x
  float4 r1;  // Tv.y Tv.z Tw.x Tw.y
  float4 r2;  // Tw.z cx cy opacity
  float4 r3;  // n.x n.y n.z r
  float4 r4;  // g b C lp2   | footprint of {alpha >= 1/255}: the ellipse A dx^2 + 2B dx dy + C dy^2 <= 1 about (ex, ey)
  float4 r5;  // ex ey A B   | united with the disc |p - (cx,cy)|^2 <= lp2; A == 0: unknown, never cull
};
static_assert(sizeof(Surfel) == 96, "Surfel must be 96 bytes");

// Exact culling for surfels.  alpha >= 1/255 needs min(rho3d, rho2d) <= kk = 2 ln(255 o).  {rho3d <= kk} is the
// projection of the surfel's uv-disc of radius sqrt(kk): with p = (x Tw - Tu) x (y Tw - Tv) linear in the pixel,
// rho3d = (p0^2 + p1^2) / p2^2, so the region is the conic p0^2 + p1^2 - kk p2^2 <= 0 — an ellipse whenever the disc
// stays in front of the camera; preprocess2d_kernel normalises it (with 1% + 0.02 of slack on kk).  {rho2d <= kk} is
// a disc about the low-pass centre.  A pixel box that neither reaches cannot hold a contributing pixel, so dropping
// the (box, surfel) pair changes no output bit.
__device__ __forceinline__ bool surfel_reaches_box(float cx, float cy, const float4 r4, const float4 r5, float bx0, float bx1,
                                                   float by0, float by1) {
  if (r5.z == 0.0f) return true;
  const float ddx = fmaxf(fmaxf(bx0 - cx, cx - bx1), 0.0f), ddy = fmaxf(fmaxf(by0 - cy, cy - by1), 0.0f);
  if (ddx * ddx + ddy * ddy <= r4.w) return true;
  return conic_min_over_box(r5.x, r5.y, r5.z, r5.w, r4.z, bx0, bx1, by0, by1) <= 1.0f;
}

// The ray-surfel intersection in linear form.  With k = x Tw - Tu, l = y Tw - Tv the reference intersects with
// p = k x l and s = (p0, p1) / p2.  p is LINEAR in the pixel, and p . Tw = det[Tu; Tv; Tw] =: D for every pixel, so
// the hit depth s0 Tw0 + s1 Tw1 + Tw2 = D / p2.  A wave expands the form about the CENTRE (bxc, byc) OF ITS 8x8 BLOCK:
// with kb = bxc Tw - Tu, lb = byc Tw - Tv (each component ONE fma, so the near-cancellation of bxc Tw2 against Tu2
// costs a single rounding of the small result),
//     p(x, y) = (x - bxc) pa + (y - byc) pb + pc,    pa = Tv x Tw,  pb = Tw x Tu,  pc = kb x lb,
// and (x - bxc, y - byc) is a per-lane constant in {-3.5 .. 3.5}: six FMAs per pixel, no reciprocal for the depth (nor
// for 1 / depth: p2 / D).  Expanded about the image origin instead (pc = Tu x Tv, round 1) p0 and p1 were differences
// of terms ~10^2 times their size, and 2 % of random scenes held a surfel whose gradient missed the oracle's by more
// than its tolerance.  The lane that inserts a surfel into a wave's ring computes pa, pb, pc, D once.
// The backward accumulates the gradients of (pa, pb, pc, D) about ONE point per surfel whatever the block - its centre
// (cx, cy) clamped into the image, (ex, ey) - as products of dp with (x - ex, y - ey, 1); preprocess2d_backward_kernel
// chains them back to T with pc = (ex Tw - Tu) x (ey Tw - Tv), (ex, ey) held fixed (p as a function of T does not
// depend on where it is expanded).  A splat-centred frame keeps those sums and their cross products with T free of
// the (x, y)-weighted against (cx, cy)-weighted cancellation of the origin form; the clamp keeps a centre far outside
// the image (a large surfel seen from close by) from re-creating it.
struct SurfelLin { float4 e0, e1, e2, e3; };   // (pa, pb0) (pb1, pb2, pc0, pc1) (pc2, D, cx, cy) (log2 o, Tw2, 1/D, 1/Tw2)
__device__ __forceinline__ SurfelLin surfel_lin(const float4 r0, const float4 r1, const float4 r2, float bxc, float byc) {
#pragma clang fp contract(off)
  const float Tu[3] = {r0.x, r0.y, r0.z}, Tv[3] = {r0.w, r1.x, r1.y}, Tw[3] = {r1.z, r1.w, r2.x};
  float pa[3], pb[3], pc[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    pa[i] = __builtin_fmaf(Tv[j], Tw[k], -(Tv[k] * Tw[j]));
    pb[i] = __builtin_fmaf(Tw[j], Tu[k], -(Tw[k] * Tu[j]));
  }
  float kc[3], lc[3];
#pragma unroll
  for (int i = 0; i < 3; i++) { kc[i] = __builtin_fmaf(bxc, Tw[i], -Tu[i]); lc[i] = __builtin_fmaf(byc, Tw[i], -Tv[i]); }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    pc[i] = __builtin_fmaf(kc[j], lc[k], -(kc[k] * lc[j]));
  }
  const float D = __builtin_fmaf(Tu[0], pa[0], __builtin_fmaf(Tu[1], pa[1], Tu[2] * pa[2]));
  SurfelLin L;
  L.e0 = make_float4(pa[0], pa[1], pa[2], pb[0]);
  L.e1 = make_float4(pb[1], pb[2], pc[0], pc[1]);
  L.e2 = make_float4(pc[2], D, r2.y, r2.z);
  L.e3 = make_float4(__builtin_amdgcn_logf(r2.w), Tw[2], __builtin_amdgcn_rcpf(D), __builtin_amdgcn_rcpf(Tw[2]));
  return L;
}

struct Eval2 { float s0, s1, pz, rz, dx, dy, depth, rdepth, Go, alpha; bool use3d; };
// Same decisions in forward and backward: every product-sum is written as an explicit fma and contraction is off, so
// the two kernels cannot round the intersection differently.  Go = opacity * G (alpha before the 0.99 clamp).
__device__ __forceinline__ bool eval_surfel(const float4 e0, const float4 e1, const float4 e2, const float4 e3, float qx,
                                            float qy, float pxf, float pyf, Eval2 &h) {   // (qx, qy) = pixel - block centre
#pragma clang fp contract(off)
  const float p0 = __builtin_fmaf(e0.x, qx, __builtin_fmaf(e0.w, qy, e1.z));
  const float p1 = __builtin_fmaf(e0.y, qx, __builtin_fmaf(e1.x, qy, e1.w));
  h.pz = __builtin_fmaf(e0.z, qx, __builtin_fmaf(e1.y, qy, e2.x));
  h.rz = __builtin_amdgcn_rcpf(h.pz);
  h.s0 = p0 * h.rz; h.s1 = p1 * h.rz;
  const float rho3d = __builtin_fmaf(h.s0, h.s0, h.s1 * h.s1);
  h.dx = e2.z - pxf; h.dy = e2.w - pyf;
  const float rho2d = kFilterInvSq * __builtin_fmaf(h.dx, h.dx, h.dy * h.dy);
  h.use3d = rho3d <= rho2d;
  const float rho = fminf(rho3d, rho2d);            // rho2d is finite, so a NaN / inf rho3d (pz == 0) falls back to it
  h.depth = h.use3d ? e2.y * h.rz : e3.y;
  h.rdepth = h.use3d ? h.pz * e3.z : e3.w;          // 1 / depth without a reciprocal
  h.Go = __builtin_amdgcn_exp2f(__builtin_fmaf(-0.5f * 1.4426950408889634f, rho, e3.x));
  h.alpha = fminf(kAlphaMax, h.Go);
  return (h.pz != 0.0f) & (h.depth >= kNearZ) & (h.alpha >= kAlphaMin);
}

}  // namespace scorp
