// gs2d_pergaussian.hip — the two per-surfel (one thread per surfel) kernels of the 2DGS path for gfx950, the twins of
// gs3d_pergaussian.hip:
//   preprocess2d          : splat-to-pixel transform T, cull, tile rectangle, exact footprint, SH -> RGB   (forward)
//   preprocess2d_backward : the blend backward's twenty accumulators -> gradients of the call arguments    (backward)
// Arithmetic follows oracle/gs2d_oracle.c: each surfel is a 3x3 matrix T (rows Tu,Tv,Tw) mapping its local (u,v,1) to
// (x*w, y*w, w) in pixels.  What the two kinds' per-primitive kernels share (SH staging and evaluation, activations, the
// fused Adam pieces, quat_grad, iso_scale_grad) is in pergaussian.hpp.
#include "pergaussian.hpp"
#include "surfel.hpp"

namespace scorp {
namespace {

struct Pg2Args {
  int N, K, W, H, tiles_x, tiles_y, raw, count_with_atomics;   // (H, tiles_y: of ONE view)
  int views;   // stacked views (ScorpGs3dInputs.num_views): blockIdx.y = view, records of virtual surfel view * N + i
  float scale_mod;
  const float *view, *proj, *campos;
  const float *means3D, *shs, *shs_rest, *colors_precomp, *opacities, *scales, *rotations, *transmat;
};

__device__ __forceinline__ void pixel_rows(const float *pm, int W, int H, float Q[3][4]) {
#pragma clang fp contract(off)   // the splat-to-pixel transform feeds ceil(extent): same roundings as the CPU oracle
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const float p0 = pm[c * 4 + 0], p1 = pm[c * 4 + 1], p3 = pm[c * 4 + 3];
    Q[0][c] = 0.5f * W * p0 + 0.5f * (W - 1) * p3;
    Q[1][c] = 0.5f * H * p1 + 0.5f * (H - 1) * p3;
    Q[2][c] = p3;
  }
}

__device__ __forceinline__ void quat_R(float4 q, float *R) {
#pragma clang fp contract(off)
  const float r = q.x, x = q.y, y = q.z, z = q.w;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - r * z);     R[2] = 2 * (x * z + r * y);
  R[3] = 2 * (x * y + r * z);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - r * x);
  R[6] = 2 * (x * z - r * y);     R[7] = 2 * (y * z + r * x);     R[8] = 1 - 2 * (x * x + y * y);
}

// ---------------------------------------------------------------------------------------------------------
// LIN: full workgroups of the training layout (dc / rest split, K = 16, scales + rotations) - parameters fetched with
// untracked loads AHEAD of the SH stream (direct global -> LDS loads) and picked up at vmcnt(12); see pergaussian.hpp.
template <int DEG, bool SPLIT, bool LIN>
__device__ __forceinline__ void preprocess2d_body(const Pg2Args &a, float *s_sh, Surfel *__restrict__ rec,
                                                  BinRec *__restrict__ bin, uint64_t *__restrict__ tile_mask,
                                                  int32_t *__restrict__ radii, uint32_t *__restrict__ tile_count) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool active = LIN || i < a.N;
  constexpr int NFL = 3 * (DEG + 1) * (DEG + 1);
  const size_t i0 = (size_t)blockIdx.x * 256;
  const int nrows_f = LIN ? 256 : min(256, a.N - (int)i0);
  constexpr bool lin = LIN;
  float pre[11];   // LIN: means 0-2, rotation 3-6, scale 7-8, opacity 10
  if constexpr (LIN) {
    RawParams r;
    raw_issue_params<2>(r, a.means3D + 3 * (size_t)i, a.rotations + 4 * (size_t)i, a.scales + 2 * (size_t)i, a.opacities + i);
    // (nontemporal for one view; a stacked launch re-reads the rows once per view, from L2: see preprocess_body, gs3d_pergaussian.hip)
    if (a.views <= 1) stage_sh_linear_async<2>(s_sh, a.shs, a.shs_rest, i0);
    else stage_sh_linear_async<0>(s_sh, a.shs, a.shs_rest, i0);
    raw_take_params(r, pre);
  }
  const int view = a.views > 1 ? (int)blockIdx.y : 0;   // workgroup-uniform: the matrices stay scalar loads
  const CFloat *cv = (const CFloat *)a.view + 16 * view, *cp = (const CFloat *)a.proj + 16 * view;
  float vm[16], pm[16];
#pragma unroll
  for (int q = 0; q < 16; q++) { vm[q] = cv[q]; pm[q] = cp[q]; }   // scalar cache
  BinRec br;
  br.x0 = br.y0 = br.x1 = br.y1 = 0; br.depth_bits = 0; br.radius = 0;
  bool vis = false;
  float T[9], nv[3] = {0, 0, 1}, p[3] = {0, 0, 0}, cx = 0, cy = 0, op = 0, depth = 0, mult = 1;
  float eA = 0, eB = 0, eC = 0, ex = 0, ey = 0, lp2 = 0;
  uint64_t mask = kMaskAll;
  int radius = 0, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
  if (active) {
    if constexpr (LIN) { p[0] = pre[0]; p[1] = pre[1]; p[2] = pre[2]; }
    else { p[0] = a.means3D[3 * (size_t)i]; p[1] = a.means3D[3 * (size_t)i + 1]; p[2] = a.means3D[3 * (size_t)i + 2]; }
    const float pvx = vm[0] * p[0] + vm[4] * p[1] + vm[8] * p[2] + vm[12];
    const float pvy = vm[1] * p[0] + vm[5] * p[1] + vm[9] * p[2] + vm[13];
    depth = __builtin_fmaf(vm[10], p[2], __builtin_fmaf(vm[6], p[1], __builtin_fmaf(vm[2], p[0], vm[14])));
    if (depth > kNearZ) {
      if (!LIN && a.transmat) {
#pragma unroll
        for (int q = 0; q < 9; q++) T[q] = a.transmat[9 * (size_t)i + q];
      } else {
        float Q[3][4], R[9], invn;
        pixel_rows(pm, a.W, a.H, Q);
        const float4 q_in = LIN ? make_float4(pre[3], pre[4], pre[5], pre[6]) : reinterpret_cast<const float4 *>(a.rotations)[i];
        quat_R(act_quat(q_in, a.raw, &invn), R);
        const float sx = a.scale_mod * act_scale(LIN ? pre[7] : a.scales[2 * (size_t)i], a.raw),
                    sy = a.scale_mod * act_scale(LIN ? pre[8] : a.scales[2 * (size_t)i + 1], a.raw);
#pragma unroll
        for (int r = 0; r < 3; r++) {
          T[r * 3 + 0] = sx * (Q[r][0] * R[0] + Q[r][1] * R[3] + Q[r][2] * R[6]);
          T[r * 3 + 1] = sy * (Q[r][0] * R[1] + Q[r][1] * R[4] + Q[r][2] * R[7]);
          T[r * 3 + 2] = Q[r][0] * p[0] + Q[r][1] * p[1] + Q[r][2] * p[2] + Q[r][3];
        }
#pragma unroll
        for (int r = 0; r < 3; r++) nv[r] = vm[0 * 4 + r] * R[2] + vm[1 * 4 + r] * R[5] + vm[2 * 4 + r] * R[8];
      }
      const float cosv = -(pvx * nv[0] + pvy * nv[1] + depth * nv[2]);
      const float *Tu = T, *Tv = T + 3, *Tw = T + 6;
      const float c2 = kCutoff * kCutoff;
      const float dd = c2 * Tw[0] * Tw[0] + c2 * Tw[1] * Tw[1] + -1.0f * Tw[2] * Tw[2];
      if (cosv != 0.0f && dd != 0.0f) {
        mult = cosv > 0.0f ? 1.0f : -1.0f;
        const float f0 = c2 / dd, f1 = c2 / dd, f2 = -1.0f / dd;
        cx = f0 * Tu[0] * Tw[0] + f1 * Tu[1] * Tw[1] + f2 * Tu[2] * Tw[2];
        cy = f0 * Tv[0] * Tw[0] + f1 * Tv[1] * Tw[1] + f2 * Tv[2] * Tw[2];
        const float tx = f0 * Tu[0] * Tu[0] + f1 * Tu[1] * Tu[1] + f2 * Tu[2] * Tu[2];
        const float ty = f0 * Tv[0] * Tv[0] + f1 * Tv[1] * Tv[1] + f2 * Tv[2] * Tv[2];
        const float extx = sqrtf(fmaxf(kExtentFloor, cx * cx - tx)), exty = sqrtf(fmaxf(kExtentFloor, cy * cy - ty));
        radius = (int)ceilf(fmaxf(fmaxf(extx, exty), kCutoff * kFilterSize));
        x0 = min(a.tiles_x, max(0, (int)((cx - radius) / kTile)));
        y0 = min(a.tiles_y, max(0, (int)((cy - radius) / kTile)));
        x1 = min(a.tiles_x, max(0, (int)((cx + radius + kTile - 1) / kTile)));
        y1 = min(a.tiles_y, max(0, (int)((cy + radius + kTile - 1) / kTile)));
        if ((x1 - x0) * (y1 - y0) > 0) {
          vis = true;
          op = act_opacity(LIN ? pre[10] : a.opacities[i], a.raw);
          // footprint of {alpha >= 1/255} (see surfel_reaches_box), in the frame centred on (cx, cy)
          const float kk = 1.01f * 2.0f * logf(fmaxf(255.0f * op, 1.0f)) + 0.02f;
          lp2 = 0.5f * kk;
          const float ddk = kk * Tw[0] * Tw[0] + kk * Tw[1] * Tw[1] - Tw[2] * Tw[2];
          if (ddk < 0.0f) {  // the uv-disc of radius sqrt(kk) stays in front of the camera plane: bounded projection
            const float pa[3] = {Tv[1] * Tw[2] - Tv[2] * Tw[1], Tv[2] * Tw[0] - Tv[0] * Tw[2], Tv[0] * Tw[1] - Tv[1] * Tw[0]};
            const float pb[3] = {Tw[1] * Tu[2] - Tw[2] * Tu[1], Tw[2] * Tu[0] - Tw[0] * Tu[2], Tw[0] * Tu[1] - Tw[1] * Tu[0]};
            float pc[3] = {Tu[1] * Tv[2] - Tu[2] * Tv[1], Tu[2] * Tv[0] - Tu[0] * Tv[2], Tu[0] * Tv[1] - Tu[1] * Tv[0]};
#pragma unroll
            for (int q = 0; q < 3; q++) pc[q] += pa[q] * cx + pb[q] * cy;
            const float Mxx = pa[0] * pa[0] + pa[1] * pa[1] - kk * pa[2] * pa[2];
            const float Mxy = pa[0] * pb[0] + pa[1] * pb[1] - kk * pa[2] * pb[2];
            const float Myy = pb[0] * pb[0] + pb[1] * pb[1] - kk * pb[2] * pb[2];
            const float Mx1 = pa[0] * pc[0] + pa[1] * pc[1] - kk * pa[2] * pc[2];
            const float My1 = pb[0] * pc[0] + pb[1] * pc[1] - kk * pb[2] * pc[2];
            const float M11 = pc[0] * pc[0] + pc[1] * pc[1] - kk * pc[2] * pc[2];
            const float dM = Mxx * Myy - Mxy * Mxy;
            // A surfel seen nearly edge-on projects to a sliver (a major axis of 100 px on a minor axis of 0.05 px occurs):
            // rotated on the pixel grid, its conic has Mxx Myy ~ Mxy^2 and fp32 leaves dM - and with it the centre and the
            // normalisation - no digits, which dropped blocks the sliver does cross (an isolated pixel of alpha 0.24 in
            // a fuzz case).  The footprint is trusted only while every difference below keeps at least two digits;
            // otherwise the surfel is never culled inside its rectangle (the published rasterizer's own behaviour).
#ifndef SCORP_2D_SOUND_M
#define SCORP_2D_SOUND_M 1e-3f
#endif
#ifndef SCORP_2D_SOUND_D
#define SCORP_2D_SOUND_D 1e-4f
#endif
            const bool sound = Mxx > SCORP_2D_SOUND_M * (pa[0] * pa[0] + pa[1] * pa[1] + kk * pa[2] * pa[2]) &&
                               Myy > SCORP_2D_SOUND_M * (pb[0] * pb[0] + pb[1] * pb[1] + kk * pb[2] * pb[2]) &&
                               dM > SCORP_2D_SOUND_D * (Mxx * Myy + Mxy * Mxy);
            if (sound) {
              const float ox = (My1 * Mxy - Mx1 * Myy) / dM, oy = (Mx1 * Mxy - My1 * Mxx) / dM;
              const float t1 = Mx1 * ox, t2 = My1 * oy;
              const float F = M11 + t1 + t2;
              // trust the normalisation only when F did not lose its digits to cancellation and the centre is sane
              if (F < 0.0f && -F > 1e-3f * (fabsf(M11) + fabsf(t1) + fabsf(t2)) && fabsf(ox) < 4096.0f && fabsf(oy) < 4096.0f) {
                const float nf = -1.0f / F;
                eA = Mxx * nf; eB = Mxy * nf; eC = Myy * nf; ex = cx + ox; ey = cy + oy;
                if (!(eA > 0.0f && eC > 0.0f && eA < 3.0e38f && eC < 3.0e38f)) eA = eB = eC = 0.0f;
              }
            }
          }
          if (eA > 0.0f && x1 - x0 <= 8 && y1 - y0 <= 8) {
            const float4 t4 = make_float4(0.0f, 0.0f, eC, lp2), t5 = make_float4(ex, ey, eA, eB);
            mask = 0;
            for (int ty = y0; ty < y1; ty++)
              for (int tx = x0; tx < x1; tx++)
                if (surfel_reaches_box(cx, cy, t4, t5, (float)(tx * kTile), (float)(tx * kTile + kTile - 1), (float)(ty * kTile),
                                       (float)(ty * kTile + kTile - 1)))
                  mask |= 1ull << ((ty - y0) * 8 + (tx - x0));
          }
        }
      }
    }
  }
  float rgb[3] = {0.0f, 0.0f, 0.0f};
  int clamp_bits = 0;
  if (a.shs) {
    if (lin) stage_sh_wait();
    if (__syncthreads_or(vis ? 1 : 0)) {
      if (!lin) {
        stage_sh_rows<NFL, SPLIT>(s_sh, a.shs, a.shs_rest, a.K, i0, nrows_f);
        __syncthreads();
      }
      if (vis) {
        const CFloat *cc = (const CFloat *)a.campos + 3 * view;
        const float dx = p[0] - cc[0], dy = p[1] - cc[1], dz = p[2] - cc[2];
        const float inv = 1.0f / sqrtf(dx * dx + dy * dy + dz * dz);
        sh_row_to_rgb<DEG>(sh_row(s_sh, threadIdx.x, lin), dx * inv, dy * inv, dz * inv, rgb);
#pragma unroll
        for (int q = 0; q < 3; q++) {
          if (rgb[q] < 0.0f) clamp_bits |= 1 << q;
          rgb[q] = fmaxf(rgb[q], 0.0f);
        }
      }
    }
  } else if (vis) {
#pragma unroll
    for (int q = 0; q < 3; q++) rgb[q] = a.colors_precomp[3 * (size_t)i + q];
  }
  if (!active) return;
  const int row = view * a.N + i;   // the virtual surfel of the stacked image (validate: views x N < 2^31)
  if (view > 0) {   // into the view's band of the stacked image: only the TILE rectangle moves (the tile mask is relative to
                    // it); the record keeps the view's own pixel coordinates and the blend kernel works band-locally
                    // (see preprocess_body, gs3d_pergaussian.hip)
    y0 += view * a.tiles_y; y1 += view * a.tiles_y;
  }
  int radius_out = 0;
  if (vis) {
    float4 *dst = reinterpret_cast<float4 *>(rec + row);
    dst[0] = make_float4(T[0], T[1], T[2], T[3]);
    dst[1] = make_float4(T[4], T[5], T[6], T[7]);
    dst[2] = make_float4(T[8], cx, cy, op);
    dst[3] = make_float4(mult * nv[0], mult * nv[1], mult * nv[2], rgb[0]);
    dst[4] = make_float4(rgb[1], rgb[2], eC, lp2);
    dst[5] = make_float4(ex, ey, eA, eB);
    br.x0 = (uint16_t)x0; br.y0 = (uint16_t)y0; br.x1 = (uint16_t)x1; br.y1 = (uint16_t)y1;
    br.depth_bits = __float_as_uint(depth);
    br.radius = radius | (clamp_bits << kClampShift) | ((mult < 0.0f ? 1 : 0) << kFlipBit);
    radius_out = radius;
    if (a.count_with_atomics)
      for_each_tile(x0, y0, x1, y1, mask, a.tiles_x, [&](int t) { atomicAdd(&tile_count[t], 1u); });
  }
  reinterpret_cast<uint4 *>(bin)[row] = *reinterpret_cast<const uint4 *>(&br);
  tile_mask[row] = mask;
  radii[row] = radius_out;
}

template <int DEG, bool SPLIT>
__global__ void __launch_bounds__(256)
preprocess2d_kernel(Pg2Args a, Surfel *__restrict__ rec, BinRec *__restrict__ bin, uint64_t *__restrict__ tile_mask,
                    int32_t *__restrict__ radii, uint32_t *__restrict__ tile_count) {
  __shared__ __attribute__((aligned(16))) float s_sh[256 * kShStride];   // direct global->LDS loads land 16-byte words
  if constexpr (SPLIT && DEG == 3) {
    if (a.shs != nullptr && a.K == 16 && !a.transmat && a.N - (int)blockIdx.x * 256 >= 256) {
      preprocess2d_body<DEG, SPLIT, true>(a, s_sh, rec, bin, tile_mask, radii, tile_count);
      return;
    }
  }
  preprocess2d_body<DEG, SPLIT, false>(a, s_sh, rec, bin, tile_mask, radii, tile_count);
}

// ---------------------------------------------------------------------------------------------------------
// LIN: full workgroups of the training layout.  Everything a surfel needs (radius and depth words, the 20-float
// accumulator row, the nine floats of its transform, its parameters) is requested unconditionally BEFORE the SH stream is
// issued, so that one memory latency covers it all instead of the chain radius -> visible? -> rows -> parameters behind
// the stream.  Plain 16-byte loads here: the 44 dwords as untracked one-dword loads (the forward's way, which would also
// let the maths start before the stream has landed) cost more in the texture pipe than they gain (121 vs 118 us).
// ISO: the isotropic regulariser's gradient (train_2dgs.py:136-139 over the [N,2] scales) joins the scaling gradient of EVERY
// surfel of the block, visible or not; iso_k = lambda_isotropic / (4 N).  The plain instantiations do not know it exists.
template <int DEG, bool SPLIT, bool LIN, bool ISO = false>
__device__ __forceinline__ void preprocess2d_backward_body(const Pg2Args &a, float *s_sh, const Surfel *__restrict__ rec,
                                                           const BinRec *__restrict__ bin, const float *__restrict__ acc,
                                                           const ScorpGs3dGrads &g, const AdamEpi &ad, float iso_k = 0.0f) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool active = LIN || i < a.N;
  const size_t i0 = (size_t)blockIdx.x * 256;
  const int nrows = LIN ? 256 : min(256, a.N - (int)i0);
  constexpr int NFL = 3 * (DEG + 1) * (DEG + 1);
  // LIN: pre = means 0-2, rotation 3-6, scale 7-8, opacity 10 | acc_lo = accumulators 0-10 | acc_hi = accumulators
  // 11-19 in slots 0-8, radius word in slot 10 | rec_lo = transform 0-8, depth word in slot 10
  float pre[11], acc_lo[11], acc_hi[11], rec_lo[11];
  float lin_cx = 0.0f, lin_cy = 0.0f, lin_op = 1.0f;   // LIN: the surfel's centre and opacity (record r2.y, r2.z, r2.w)
  int32_t rad_bits = 0;
  if constexpr (LIN) {
    static_assert(kAcc2Stride == 20, "accumulator row of 20 floats");
    const float4 *ap = reinterpret_cast<const float4 *>(acc + (size_t)i * kAcc2Stride);
    const float4 *rp = reinterpret_cast<const float4 *>(rec + i);
    const uint4 bw = reinterpret_cast<const uint4 *>(bin)[i];
    const float4 a0 = ap[0], a1 = ap[1], a2 = ap[2], a3 = ap[3], a4 = ap[4], r0 = rp[0], r1 = rp[1];
    const float4 r2v = rp[2];   // Tw.z, cx, cy, (opacity)
    const float4 q_in = reinterpret_cast<const float4 *>(a.rotations)[i];
    const float s_in0 = a.scales[2 * (size_t)i], s_in1 = a.scales[2 * (size_t)i + 1];
    pre[0] = a.means3D[3 * (size_t)i]; pre[1] = a.means3D[3 * (size_t)i + 1]; pre[2] = a.means3D[3 * (size_t)i + 2];
    pre[10] = a.opacities[i];
    // (nontemporal unless the optimizer step in the epilogue reads the rows again: see preprocess_backward_body, gs3d_pergaussian.hip)
    if (!(SPLIT && ad.on != 0)) stage_sh_linear_async<2>(s_sh, a.shs, a.shs_rest, i0);
    else stage_sh_linear_async<0>(s_sh, a.shs, a.shs_rest, i0);
    pre[3] = q_in.x; pre[4] = q_in.y; pre[5] = q_in.z; pre[6] = q_in.w; pre[7] = s_in0; pre[8] = s_in1;
    acc_lo[0] = a0.x; acc_lo[1] = a0.y; acc_lo[2] = a0.z; acc_lo[3] = a0.w; acc_lo[4] = a1.x; acc_lo[5] = a1.y; acc_lo[6] = a1.z;
    acc_lo[7] = a1.w; acc_lo[8] = a2.x; acc_lo[9] = a2.y; acc_lo[10] = a2.z;
    acc_hi[0] = a2.w; acc_hi[1] = a3.x; acc_hi[2] = a3.y; acc_hi[3] = a3.z; acc_hi[4] = a3.w; acc_hi[5] = a4.x; acc_hi[6] = a4.y;
    acc_hi[7] = a4.z; acc_hi[8] = a4.w;
    rec_lo[0] = r0.x; rec_lo[1] = r0.y; rec_lo[2] = r0.z; rec_lo[3] = r0.w; rec_lo[4] = r1.x; rec_lo[5] = r1.y; rec_lo[6] = r1.z;
    rec_lo[7] = r1.w; rec_lo[8] = r2v.x;
    lin_cx = r2v.y; lin_cy = r2v.z; lin_op = r2v.w;
    rec_lo[10] = __uint_as_float(bw.z);   // BinRec: x0y0 | x1y1 | depth word | radius word
    acc_hi[10] = __uint_as_float(bw.w);
    rad_bits = __float_as_int(acc_hi[10]);
  } else {
    rad_bits = active ? bin[i].radius : 0;
  }
  const bool visible = (rad_bits & kRadiusMask) != 0;
  // the optimizer step inside the view (scorp_gs2d_train_view with `adam`; see preprocess_backward_body in gs3d_pergaussian.hip)
  const bool adam_on = SPLIT && ad.on != 0;
  const bool adam_sh = adam_on && (ad.m[1] != nullptr || ad.m[2] != nullptr);
  const bool want_sh_grad = a.shs != nullptr && (g.shs != nullptr || adam_sh);
  bool staged = false;
  constexpr bool lin = LIN;
  if (a.shs) {
    if constexpr (lin) {
      staged = true;
    } else {
      if (__syncthreads_or(visible ? 1 : 0)) {
        stage_sh_rows<NFL, SPLIT>(s_sh, a.shs, a.shs_rest, a.K, i0, nrows);
        staged = true;
      }
      __syncthreads();
    }
  }
  float shx = 0, shy = 0, shz = 0, shinv = 0, gr3[3] = {0, 0, 0};
  float vm[16], pm[16];
#pragma unroll
  for (int q = 0; q < 16; q++) { vm[q] = ((const CFloat *)a.view)[q]; pm[q] = ((const CFloat *)a.proj)[q]; }   // scalar cache
  float gm[3] = {0, 0, 0}, gs[2] = {0, 0}, gq[4] = {0, 0, 0, 0}, gT[9], gm2[2] = {0, 0}, grgb[3] = {0, 0, 0}, g_op = 0;
#pragma unroll
  for (int q = 0; q < 9; q++) gT[q] = 0.0f;
  const ShRow row = sh_row(s_sh, threadIdx.x, lin);
  if (visible) {
    float4 a0, a1, a2, a3, a4, r0, r1, r2;
    if constexpr (LIN) {
      a0 = make_float4(acc_lo[0], acc_lo[1], acc_lo[2], acc_lo[3]); a1 = make_float4(acc_lo[4], acc_lo[5], acc_lo[6], acc_lo[7]);
      a2 = make_float4(acc_lo[8], acc_lo[9], acc_lo[10], acc_hi[0]); a3 = make_float4(acc_hi[1], acc_hi[2], acc_hi[3], acc_hi[4]);
      a4 = make_float4(acc_hi[5], acc_hi[6], acc_hi[7], acc_hi[8]);
      r0 = make_float4(rec_lo[0], rec_lo[1], rec_lo[2], rec_lo[3]); r1 = make_float4(rec_lo[4], rec_lo[5], rec_lo[6], rec_lo[7]);
      r2 = make_float4(rec_lo[8], lin_cx, lin_cy, lin_op);
    } else {
      const float4 *ap = reinterpret_cast<const float4 *>(acc + (size_t)i * kAcc2Stride);
      a0 = ap[0]; a1 = ap[1]; a2 = ap[2]; a3 = ap[3]; a4 = ap[4];
      const float4 *rp = reinterpret_cast<const float4 *>(rec + i);
      r0 = rp[0]; r1 = rp[1]; r2 = rp[2];
    }
    const float ga[3] = {a0.x, a0.y, a0.z}, gb[3] = {a0.w, a1.x, a1.y}, gc[3] = {a1.z, a1.w, a2.x};
    const float gD = a2.y, gTw2 = a2.z, gx = a2.w, gy = a3.x;
    const float gn[3] = {a3.y, a3.z, a3.w};
    g_op = a4.x / r2.w;   // the blend kernel summed opacity * G * dL/dalpha
    grgb[0] = a4.y; grgb[1] = a4.z; grgb[2] = a4.w;
    const float Tu[3] = {r0.x, r0.y, r0.z}, Tv[3] = {r0.w, r1.x, r1.y}, Tw[3] = {r1.z, r1.w, r2.x};
    // the blend kernels hand over the gradients of the linear form p = (x - ex) pa + (y - ey) pb + pc, depth = D / p.z
    // (see surfel_lin): pa = Tv x Tw, pb = Tw x Tu, pc = kc x lc with kc = ex Tw - Tu, lc = ey Tw - Tv, D = Tu . pa,
    // (ex, ey) = the centre clamped into the image, held fixed.  For c = u x v: dL/du = v x g, dL/dv = g x u.
    const float ecx = fminf(fmaxf(r2.y, 0.0f), (float)(a.W - 1)), ecy = fminf(fmaxf(r2.z, 0.0f), (float)(a.H - 1));
    float kc[3], lc[3], gkc[3], glc[3];
#pragma unroll
    for (int q = 0; q < 3; q++) { kc[q] = __builtin_fmaf(ecx, Tw[q], -Tu[q]); lc[q] = __builtin_fmaf(ecy, Tw[q], -Tv[q]); }
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int j = (q + 1) % 3, k = (q + 2) % 3;
      gkc[q] = lc[j] * gc[k] - lc[k] * gc[j];   // d/dkc = lc x gc
      glc[q] = gc[j] * kc[k] - gc[k] * kc[j];   // d/dlc = gc x kc
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const int j = (q + 1) % 3, k = (q + 2) % 3;
      const float pa_q = Tv[j] * Tw[k] - Tv[k] * Tw[j], pb_q = Tw[j] * Tu[k] - Tw[k] * Tu[j], tuv_q = Tu[j] * Tv[k] - Tu[k] * Tv[j];
      gT[q] = (gb[j] * Tw[k] - gb[k] * Tw[j]) - gkc[q] + gD * pa_q;                                  // d/dTu
      gT[3 + q] = (Tw[j] * ga[k] - Tw[k] * ga[j]) - glc[q] + gD * pb_q;                              // d/dTv
      gT[6 + q] = (ga[j] * Tv[k] - ga[k] * Tv[j]) + (Tu[j] * gb[k] - Tu[k] * gb[j]) + (ecx * gkc[q] + ecy * glc[q])
                  + gD * tuv_q;                                                                      // d/dTw (dD/dTw = Tu x Tv)
    }
    gT[8] += gTw2;
    const float depth = LIN ? rec_lo[10] : __uint_as_float(bin[i].depth_bits);
    gm2[0] = gT[2] * depth * 0.5f * a.W;   // densification statistic (gs2dgs/scene/gaussian_model.py:495 consumes it)
    gm2[1] = gT[5] * depth * 0.5f * a.H;
    if (gx != 0.0f || gy != 0.0f) {        // the low-pass centre is the centre of the 3-sigma box, a function of T
      const float c2 = kCutoff * kCutoff;
      const float t[3] = {c2, c2, -1.0f};
      const float dd = t[0] * Tw[0] * Tw[0] + t[1] * Tw[1] * Tw[1] + t[2] * Tw[2] * Tw[2];
      float dLdd = 0.0f;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const float f = t[q] / dd;
        gT[q] += gx * f * Tw[q];
        gT[3 + q] += gy * f * Tw[q];
        gT[6 + q] += gx * f * Tu[q] + gy * f * Tv[q];
        dLdd += (gx * Tu[q] * Tw[q] + gy * Tv[q] * Tw[q]) * f;
      }
      dLdd *= -1.0f / dd;
#pragma unroll
      for (int q = 0; q < 3; q++) gT[6 + q] += dLdd * 2.0f * t[q] * Tw[q];
    }
    if (a.raw & 1) {
      const float o = act_opacity(LIN ? pre[10] : a.opacities[i], a.raw);
      g_op *= o * (1.0f - o);
    }
    float p0, p1, p2;
    if constexpr (LIN) { p0 = pre[0]; p1 = pre[1]; p2 = pre[2]; }
    else { p0 = a.means3D[3 * (size_t)i]; p1 = a.means3D[3 * (size_t)i + 1]; p2 = a.means3D[3 * (size_t)i + 2]; }
    if (LIN || !a.transmat) {
      float Q[3][4], R[9], inv_qn;
      pixel_rows(pm, a.W, a.H, Q);
      const float4 q_in = LIN ? make_float4(pre[3], pre[4], pre[5], pre[6]) : reinterpret_cast<const float4 *>(a.rotations)[i];
      const float4 qn = act_quat(q_in, a.raw, &inv_qn);
      quat_R(qn, R);
      const float sa0 = act_scale(LIN ? pre[7] : a.scales[2 * (size_t)i], a.raw),
                  sa1 = act_scale(LIN ? pre[8] : a.scales[2 * (size_t)i + 1], a.raw);
      const float sx = a.scale_mod * sa0, sy = a.scale_mod * sa1;
      float gh[3][3];
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int c = 0; c < 3; c++) gh[j][c] = gT[0 * 3 + j] * Q[0][c] + gT[1 * 3 + j] * Q[1][c] + gT[2 * 3 + j] * Q[2][c];
#pragma unroll
      for (int c = 0; c < 3; c++) gm[c] = gh[2][c];
      const float mult = ((rad_bits >> kFlipBit) & 1) ? -1.0f : 1.0f;
      float gtn[3];
#pragma unroll
      for (int c = 0; c < 3; c++) gtn[c] = mult * (vm[c * 4 + 0] * gn[0] + vm[c * 4 + 1] * gn[1] + vm[c * 4 + 2] * gn[2]);
      float gR[9];
#pragma unroll
      for (int r = 0; r < 3; r++) { gR[r * 3 + 0] = gh[0][r] * sx; gR[r * 3 + 1] = gh[1][r] * sy; gR[r * 3 + 2] = gtn[r]; }
      gs[0] = a.scale_mod * (gh[0][0] * R[0] + gh[0][1] * R[3] + gh[0][2] * R[6]);
      gs[1] = a.scale_mod * (gh[1][0] * R[1] + gh[1][1] * R[4] + gh[1][2] * R[7]);
      if (a.raw & 2) { gs[0] *= sa0; gs[1] *= sa1; }
      quat_grad(qn, gR, a.raw, inv_qn, gq);
    }
    if (a.shs) {   // the SH part itself runs after the rows have landed in LDS (below)
      const float d0 = p0 - ((const CFloat *)a.campos)[0], d1 = p1 - ((const CFloat *)a.campos)[1], d2_ = p2 - ((const CFloat *)a.campos)[2];
      shinv = 1.0f / sqrtf(d0 * d0 + d1 * d1 + d2_ * d2_);
      shx = d0 * shinv; shy = d1 * shinv; shz = d2_ * shinv;
#pragma unroll
      for (int ch = 0; ch < 3; ch++) gr3[ch] = ((rad_bits >> (kClampShift + ch)) & 1) ? 0.0f : grgb[ch];
    }
  }
  if constexpr (ISO) {   // (pergaussian.hpp: iso_scale_grad)
    if (active && (g.scales != nullptr || (adam_on && ad.m[4] != nullptr)))
      iso_scale_grad<2>(LIN ? pre + 7 : a.scales + 2 * (size_t)i, a.raw, iso_k, gs);
  }
  if (a.shs && lin) { stage_sh_wait(); __syncthreads(); }
  AdamGeomMoments am;   // asked for here, used in the epilogue: the SH phase in between hides the latency
  if (adam_on && active && !a.transmat) {
    adam_moments_load<3>(ad, 0, 3 * (size_t)i, am.m, am.v);
    adam_moments_load<1>(ad, 3, (size_t)i, am.m + 3, am.v + 3);
    adam_moments_load<2>(ad, 4, 2 * (size_t)i, am.m + 4, am.v + 4);
    adam_moments_load<4>(ad, 5, 4 * (size_t)i, am.m + 7, am.v + 7);
  }
  if (visible && a.shs) {
    float gdir[3] = {0, 0, 0};
    sh_row_backward<DEG>(row, shx, shy, shz, gr3, want_sh_grad, gdir);
    sh_dir_to_mean(shx, shy, shz, shinv, gdir, gm);
  } else if (want_sh_grad && active) {
    sh_row_zero(row);
  }
  if (active) {
    if (g.means3D) { g.means3D[3 * (size_t)i] = gm[0]; g.means3D[3 * (size_t)i + 1] = gm[1]; g.means3D[3 * (size_t)i + 2] = gm[2]; }
    if (g.means2D) { g.means2D[3 * (size_t)i] = gm2[0]; g.means2D[3 * (size_t)i + 1] = gm2[1]; g.means2D[3 * (size_t)i + 2] = 0.0f; }
    if (g.colors_precomp) { g.colors_precomp[3 * (size_t)i] = grgb[0]; g.colors_precomp[3 * (size_t)i + 1] = grgb[1]; g.colors_precomp[3 * (size_t)i + 2] = grgb[2]; }
    if (g.opacities) g.opacities[i] = g_op;
    if (g.scales) { g.scales[2 * (size_t)i] = gs[0]; g.scales[2 * (size_t)i + 1] = gs[1]; }
    if (g.rotations) reinterpret_cast<float4 *>(g.rotations)[i] = make_float4(gq[0], gq[1], gq[2], gq[3]);
    if (g.cov3D_precomp) {
#pragma unroll
      for (int q = 0; q < 9; q++) g.cov3D_precomp[9 * (size_t)i + q] = gT[q];
    }
  }
  // Adam + the view's densification statistics where the gradient row is at hand (train_2dgs.py:189-199 over
  // gs2dgs/scene/gaussian_model.py:494-495: the statistic norms the whole means2D-gradient row, whose third component is 0)
  bool adam_go = false;
  if constexpr (SPLIT) {
    if (adam_on) {
      adam_go = !(ad.skip && *ad.skip != 0u);
      if (!adam_go && ad.skipped_counter && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(ad.skipped_counter, 1u);
      if (adam_go && active && !a.transmat) {
        float pin[11];
        if constexpr (LIN) {
#pragma unroll
          for (int q = 0; q < 11; q++) pin[q] = pre[q];
        }
        adam_leaf_pre<3>(ad, 0, const_cast<float *>(a.means3D), 3 * (size_t)i, gm, LIN ? pin : nullptr, am.m, am.v);
        adam_leaf_pre<1>(ad, 3, const_cast<float *>(a.opacities), (size_t)i, &g_op, LIN ? pin + 10 : nullptr, am.m + 3, am.v + 3);
        adam_leaf_pre<2>(ad, 4, const_cast<float *>(a.scales), 2 * (size_t)i, gs, LIN ? pin + 7 : nullptr, am.m + 4, am.v + 4);
        adam_leaf_pre<4>(ad, 5, const_cast<float *>(a.rotations), 4 * (size_t)i, gq, LIN ? pin + 3 : nullptr, am.m + 7, am.v + 7);
        if (ad.accum && visible) {
#pragma clang fp contract(off)
          const float gx = gm2[0], gy = gm2[1];
          ad.max_radii2D[i] = fmaxf(ad.max_radii2D[i], (float)(rad_bits & kRadiusMask));
          ad.accum[i] += sqrtf(gx * gx + gy * gy + 0.0f);
          ad.denom[i] += 1.0f;
        }
      }
    }
  }
  if (want_sh_grad) {
    if (!staged && active) sh_row_zero(row);
    __syncthreads();
    if (g.shs) {
      if (lin) unstage_sh_linear(s_sh, g.shs, g.shs_rest, i0);
      else unstage_sh_rows<SPLIT>(s_sh, g.shs, g.shs_rest, a.K, i0, nrows);
    }
    if constexpr (SPLIT) {
      if (adam_go && adam_sh) {
        if (lin) adam_sh_linear(ad, s_sh, const_cast<float *>(a.shs), const_cast<float *>(a.shs_rest), i0);
        else adam_sh_rows(ad, s_sh, const_cast<float *>(a.shs), const_cast<float *>(a.shs_rest), a.K, i0, nrows);
      }
    }
  }
}

template <int DEG, bool SPLIT>
__global__ void __launch_bounds__(256)
preprocess2d_backward_kernel(Pg2Args a, const Surfel *__restrict__ rec, const BinRec *__restrict__ bin,
                             const float *__restrict__ acc, ScorpGs3dGrads g, AdamEpi ad) {
  __shared__ __attribute__((aligned(16))) float s_sh[256 * kShStride];   // direct global->LDS loads land 16-byte words
  if constexpr (SPLIT && DEG == 3) {
    if (a.shs != nullptr && a.K == 16 && !a.transmat && a.N - (int)blockIdx.x * 256 >= 256) {
      preprocess2d_backward_body<DEG, SPLIT, true>(a, s_sh, rec, bin, acc, g, ad);
      return;
    }
  }
  preprocess2d_backward_body<DEG, SPLIT, false>(a, s_sh, rec, bin, acc, g, ad);
}

// The same kernel with the isotropic regulariser's gradient (split SH layout, scales + rotations: the training layout)
template <int DEG>
__global__ void __launch_bounds__(256)
preprocess2d_backward_iso_kernel(Pg2Args a, const Surfel *__restrict__ rec, const BinRec *__restrict__ bin,
                                 const float *__restrict__ acc, ScorpGs3dGrads g, AdamEpi ad, float iso_k) {
  __shared__ __attribute__((aligned(16))) float s_sh[256 * kShStride];
  if constexpr (DEG == 3) {
    if (a.K == 16 && a.N - (int)blockIdx.x * 256 >= 256) {
      preprocess2d_backward_body<DEG, true, true, true>(a, s_sh, rec, bin, acc, g, ad, iso_k);
      return;
    }
  }
  preprocess2d_backward_body<DEG, true, false, true>(a, s_sh, rec, bin, acc, g, ad, iso_k);
}

Pg2Args make_args2(const ScorpGs3dInputs *in, const StateLayout &L) {
  Pg2Args a;
  a.N = in->num_gaussians; a.K = in->sh_coeffs; a.W = in->image_width; a.H = in->image_height;
  a.tiles_x = L.tiles_x; a.tiles_y = L.tiles_y; a.raw = in->raw_params; a.count_with_atomics = L.lds_binning ? 0 : 1;
  a.scale_mod = in->scale_modifier;
  a.view = in->viewmatrix; a.proj = in->projmatrix; a.campos = in->campos;
  a.means3D = in->means3D; a.shs = in->shs; a.shs_rest = in->shs_rest; a.colors_precomp = in->colors_precomp;
  a.opacities = in->opacities; a.scales = in->scales; a.rotations = in->rotations; a.transmat = in->cov3D_precomp;
  a.views = in->num_views > 1 ? in->num_views : 1;
  if (a.views > 1) a.tiles_y = L.tiles_y / a.views;   // (L describes the stacked image)
  return a;
}

}  // namespace

void launch_preprocess2d(const ScorpGs3dInputs *in, const StateLayout &L, Surfel *rec, BinRec *bin, uint64_t *tile_mask,
                         int32_t *radii, uint32_t *tile_count, hipStream_t stream) {
  const Pg2Args a = make_args2(in, L);
  const dim3 grid((in->num_gaussians + 255) / 256, a.views), block(256);
  dispatch_sh_degree(in->shs ? in->sh_degree : 0, in->shs_rest != nullptr, [&](auto D, auto S) {
    preprocess2d_kernel<D, S><<<grid, block, 0, stream>>>(a, rec, bin, tile_mask, radii, tile_count);
  });
}

// `adam` (scorp_gs2d_train_view): the per-surfel kernel applies the optimizer step and the view's statistics itself
void launch_preprocess2d_backward(const ScorpGs3dInputs *in, const StateLayout &L, const Surfel *rec, const BinRec *bin,
                                  const float *acc, const ScorpGs3dGrads *grads, hipStream_t stream, const AdamEpi *adam,
                                  float lambda_isotropic) {
  const Pg2Args a = make_args2(in, L);
  const dim3 grid((in->num_gaussians + 255) / 256), block(256);
  const ScorpGs3dGrads g = *grads;
  AdamEpi ad;
  memset(&ad, 0, sizeof(ad));
  if (adam && in->shs_rest) ad = *adam;   // (the fused step is defined for the training layout: dc / rest split leaves)
  if (lambda_isotropic != 0.0f && a.N > 0 && in->shs && in->shs_rest && in->scales && !in->cov3D_precomp) {   // (the caller checked the layout; an empty model has no isotropic term)
    const float iso_k = (float)((double)lambda_isotropic / (4.0 * (double)a.N));
    dispatch_sh_degree(in->sh_degree, true, [&](auto D, auto) {
      preprocess2d_backward_iso_kernel<D><<<grid, block, 0, stream>>>(a, rec, bin, acc, g, ad, iso_k);
    });
    return;
  }
  dispatch_sh_degree(in->shs ? in->sh_degree : 0, in->shs_rest != nullptr, [&](auto D, auto S) {
    preprocess2d_backward_kernel<D, S><<<grid, block, 0, stream>>>(a, rec, bin, acc, g, ad);
  });
}

}  // namespace scorp
