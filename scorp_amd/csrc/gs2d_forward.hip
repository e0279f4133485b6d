// gs2d_forward.hip — 2D Gaussian splatting (surfel) path for gfx950: the blend forward with its scoring form, and the
// preprocess / render / debug entry points (the set gs3d_forward.hip holds for its kind).
//
// Replaces `diff_surfel_rasterization` as called at gs2dgs/gaussian_renderer/__init__.py:111-120 (outputs
// color[3,H,W], radii[N], allmap[7,H,W]; channel order :131-148).  Arithmetic follows oracle/gs2d_oracle.c: each
// surfel is a 3x3 matrix T (rows Tu,Tv,Tw) mapping its local (u,v,1) to (x*w, y*w, w) in pixels; a pixel intersects
// the surfel plane in uv space, alpha = o * exp(-0.5 * min(u^2+v^2, 2*|pixel - centre|^2)).
// Binning / per-tile depth sort are the 3DGS ones (binning.hip); tiles and 8x8 pixel blocks are culled by the exact
// footprint of {alpha >= 1/255} (an ellipse united with the low-pass disc).
#include <stdlib.h>

#include <type_traits>

#include "surfel.hpp"

namespace scorp {
namespace {

// ---------------------------------------------------------------------------------------------------------
// Blend kernels: one wave per 8x8 pixel block (64-thread workgroups, no workgroup barriers), the four blocks of a tile
// numbered onto the same XCD — the 2DGS twins of blend_forward_wave_kernel / blend_backward_wave_kernel.  Each lane
// of a chunk gathers one surfel of the tile's list and tests its exact footprint against the block
// (surfel_reaches_box); survivors are compacted into a per-wave LDS ring.
// ---------------------------------------------------------------------------------------------------------

// Hits per straight-line group and the waves per SIMD the kernel is held to.  Groups of 8 behind a 128-slot ring (rounds
// 2 - 3) cost 164 registers and 11.8 KB of LDS per wave: three waves per SIMD, 13 per CU by LDS.  Groups of 4 behind a
// 68-slot ring: 96 registers, 6.3 KB - five waves per SIMD.  Same box, rocprof, S6: 298 -> 272 us (render-only form
// 293 -> 262); groups of 8 squeezed into 128 registers (spills): 334; groups of 2 need more registers than groups of 4.
// The blend order does not depend on the group size (bit-identical images and hit lists).
#ifndef SCORP_2D_FGROUP
#define SCORP_2D_FGROUP 4
#endif
#ifndef SCORP_2D_FWAVES
#define SCORP_2D_FWAVES 5
#endif
constexpr int k2FChunk = 64, k2FGroup = SCORP_2D_FGROUP;
// ring: at most k2FGroup - 1 left-over hits + 64 new ones, a multiple of the group (a group's slots never wrap)
constexpr int k2FRing = (k2FChunk + k2FGroup - 1 + k2FGroup - 1) / k2FGroup * k2FGroup;

// kForBackward = false (scorp_gs2d_render_image): no cull verdicts, per-pixel state or contributor bookkeeping is left
// behind for a backward pass.
//
// Stacked views (ScorpGs3dInputs.num_views; H = the stacked height): the records hold each view's OWN pixel coordinates, so
// everything that places the block in pixel space uses the row inside its band (band_h = rows per view, a multiple of the
// tile; 0 = one view); only the output addresses and the `inside` test use the stacked row.  The band of a tile row comes
// from a scalar multiply, no division: band = ty * band_magic >> 32, band_magic = ceil(2^32 / d) for d tile rows per band
// (0 = one view; 2^32 itself for d = 1, hence 64 bits) - exact because tile rows stay below 2^16 and, with two or more
// views, d below 2^15 (ty * (band_magic * d - 2^32) < 2^31).
//
// kScore (scorp_gs2d_render_score; never with kForBackward): the twin of the 3-D kernel's scoring form.  The pose sweep
// compares alpha and the surface depth with a target and reads nothing else, so no colour, normal or distortion is
// accumulated (and their ring arrays are not filled), nothing is written to out_color / allmap, and the epilogue forms
// this pixel's |alpha - alpha*| + |surf_depth - depth*| with surf_depth = (1 - r) nan_to_num(D / alpha) + r
// nan_to_num(median) (gs2dgs/gaussian_renderer/__init__.py:139-154, r = depth_ratio), sums it over the block and leaves ONE
// float per block in block_terms[tile * 4 + quad] - plain stores, added up in a fixed order by launch_score_bands.
template <bool kForBackward, bool kScore = false>
__global__ void __launch_bounds__(64, SCORP_2D_FWAVES)
blend2d_forward_wave_kernel(const uint32_t *__restrict__ tile_start, const uint32_t *__restrict__ point_list,
                            const Surfel *__restrict__ rec, uint32_t capacity, int W, int H, int tiles_x, int tiles,
                            const float *__restrict__ bg, float *__restrict__ out_color, float *__restrict__ allmap,
                            float *__restrict__ final_T, uint32_t *__restrict__ n_contrib, uint32_t *__restrict__ hits,
                            int band_h, uint64_t band_magic, const float *__restrict__ tgt_depth = nullptr,
                            const float *__restrict__ tgt_alpha = nullptr, int score_rows = 0, float depth_ratio = 0.0f,
                            float *__restrict__ block_terms = nullptr) {
  static_assert(!(kForBackward && kScore), "the scoring form leaves nothing behind for a backward pass");
  __shared__ float4 q0[k2FRing], q1[k2FRing], q2[k2FRing], q3[k2FRing], q4[k2FRing];   // SurfelLin + (normal, r)
  __shared__ float2 q5[k2FRing];                                                          // (g, b)
  __shared__ __attribute__((aligned(16))) uint32_t q_pos[k2FRing];
  const int lane = threadIdx.x;
  BlockWave blk;
  if (!block_wave(tiles, tiles_x, blk)) return;
  const int tile = blk.tile, quad = blk.quad, bx = blk.bx, by = blk.by;
  const int byl = by - (int)(((uint64_t)(uint32_t)blk.ty * band_magic) >> 32) * band_h;   // the block's first row inside its band (scalar)
  const int px = bx + (lane & 7), py = by + (lane >> 3);
  const bool inside = px < W && py < H;
  const float pxf = (float)px, pyf = (float)(byl + (lane >> 3));
  const float bx0 = (float)bx, bx1 = (float)(bx + 7), by0 = (float)byl, by1 = (float)(byl + 7);
  const float bxc = (float)bx + 3.5f, byc = (float)byl + 3.5f;                   // the linear form's expansion point (surfel_lin)
  const float qxb = (float)(lane & 7) - 3.5f, qyb = (float)(lane >> 3) - 3.5f;   // this pixel about it
  const TileRange tr = tile_range(tile_start, tile, capacity);
  const uint32_t beg = tr.beg, n = tr.end - tr.beg;
  const float fn = kFarZ / (kFarZ - kNearZ);
  float T = inside ? 1.0f : -1.0f, C0 = 0, C1 = 0, C2 = 0, N0 = 0, N1 = 0, N2 = 0, Dp = 0, M1 = 0, M2 = 0, dist = 0, med = 0;
  uint32_t last = 0, med_c = 0;
  int head = 0, count = 0;
  uint32_t nh = 0;   // hits found so far (wave-uniform): a hit's 1-based position in the block's hit list is its `pos`
  uint32_t *my_hits = block_hit_list(hits, quad, capacity, beg);
  // The chunk's gathers (list entry -> 96-byte record) are dependent loads; software-pipelined: while chunk c is blended
  // the records of chunk c+1 and the list entries of chunk c+2 are in flight.  The entries that pass the footprint test
  // are left for the backward as the block's HIT LIST (ids, compacted, in blend order) in the pair buffer's key region
  // (dead after the sort), as in the 3-D kernels: the backward replays it and never looks at the tile's list again.
  auto fetch_id = [&](uint32_t bs) { return (bs + lane < n) ? point_list[beg + bs + lane] : 0xFFFFFFFFu; };
  auto fetch_rec = [&](uint32_t id_, float4 &a0_, float4 &a1_, float4 &a2_, float4 &a3_, float4 &a4_, float4 &a5_) {
    if (id_ != 0xFFFFFFFFu) {
      const float4 *src = reinterpret_cast<const float4 *>(rec + id_);
      a0_ = src[0]; a1_ = src[1]; a2_ = src[2];
      if constexpr (!kScore) a3_ = src[3];   // (normal, r): the score reads neither
      a4_ = src[4]; a5_ = src[5];
    }
  };
  float4 r0, r1, r2, r3, r4, r5;
  uint32_t id0 = fetch_id(0);
  fetch_rec(id0, r0, r1, r2, r3, r4, r5);
  uint32_t id1 = fetch_id(k2FChunk);
  for (uint32_t base = 0; base < n; base += k2FChunk) {
    if (__ballot(T > 0.0f) == 0) break;
    float4 nx0, nx1, nx2, nx3, nx4, nx5;   // next chunk's records
    fetch_rec(id1, nx0, nx1, nx2, nx3, nx4, nx5);
    const uint32_t id2 = fetch_id(base + 2 * k2FChunk);
    bool hit = false;
    if (id0 != 0xFFFFFFFFu) hit = surfel_reaches_box(r2.y, r2.z, r4, r5, bx0, bx1, by0, by1);
    const uint64_t m = __ballot(hit);
    if (hit) {
      const uint32_t rank = nh + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
      int qi = head + count + (int)(rank - nh);
      qi = qi >= k2FRing ? qi - k2FRing : qi;
      const SurfelLin L = surfel_lin(r0, r1, r2, bxc, byc);
      q0[qi] = L.e0; q1[qi] = L.e1; q2[qi] = L.e2; q3[qi] = L.e3;
      if constexpr (!kScore) { q4[qi] = r3; q5[qi] = make_float2(r4.x, r4.y); q_pos[qi] = rank + 1u; }
      if constexpr (kForBackward) my_hits[rank] = id0;   // (rank < n: inside this tile's slice of the region)
    }
    count += __builtin_popcountll(m);
    nh += (uint32_t)__builtin_popcountll(m);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const bool last_chunk = base + k2FChunk >= n;
    // full groups run straight-line; only a wave's final group is partial, so head stays a multiple of k2FGroup and
    // the slots of a group are head + i without wrap-around (one LDS base per array, immediate offsets)
    auto blend_group = [&](auto full, int nslots) {
      constexpr bool kFull = decltype(full)::value;
      int hv = head;
      asm volatile("" : "+v"(hv));   // keep the group's LDS bases in VGPRs
      const float4 *g0 = q0 + hv, *g1 = q1 + hv, *g2 = q2 + hv, *g3 = q3 + hv, *g4 = q4 + hv;
      const float2 *g5 = q5 + hv;
      const uint32_t *gp = q_pos + hv;
      static_assert(k2FGroup == 8 || k2FGroup == 4 || k2FGroup == 2, "positions are fetched as 16- or 8-byte LDS reads");
      uint32_t pos[k2FGroup];
      if constexpr (kScore) {   // (no positions: nothing is left for a backward)
      } else if constexpr (k2FGroup == 2) {
        const uint2 pl = *reinterpret_cast<const uint2 *>(gp);
        pos[0] = pl.x; pos[1] = pl.y;
      } else {
        const uint4 pl = *reinterpret_cast<const uint4 *>(gp);
        pos[0] = pl.x; pos[1] = pl.y; pos[2] = pl.z; pos[3] = pl.w;
        if constexpr (k2FGroup == 8) {
          const uint4 ph = *reinterpret_cast<const uint4 *>(gp + 4);
          pos[4] = ph.x; pos[5] = ph.y; pos[6] = ph.z; pos[7] = ph.w;
        }
      }
      float al[k2FGroup], dz[k2FGroup], mm[k2FGroup];
      bool okv[k2FGroup];   // (wave masks in scalar registers: the straight-line group keeps them there)
#pragma unroll
      for (int i = 0; i < k2FGroup; i++) {
        Eval2 h;
        const bool ok = eval_surfel(g0[i], g1[i], g2[i], g3[i], qxb, qyb, pxf, pyf, h) & (kFull || i < nslots);
        okv[i] = ok;
        al[i] = ok ? h.alpha : 0.0f;
        dz[i] = ok ? h.depth : 1.0f;
        if constexpr (!kScore) mm[i] = __builtin_fmaf(-fn * kNearZ, ok ? h.rdepth : 1.0f, fn);   // the backward's m_d, to the bit
      }
#pragma unroll
      for (int i = 0; i < k2FGroup; i++) {
        if (kFull || i < nslots) {  // wave-uniform
          // saturation is latched by the sign of T (see blend_forward_wave_kernel)
          if constexpr (kScore) {   // the same T, Dp and median as below, to the bit; nothing else
            const float alpha = al[i];
            const float test_T = T * (1.0f - alpha);
            const bool ok = test_T >= kTMin;
            const float w = (ok ? alpha : 0.0f) * T;
            Dp += dz[i] * w;
            med = (okv[i] & ok & (T > 0.5f)) ? dz[i] : med;
            T = ok ? test_T : -fabsf(T);
          } else {
            const float4 nr = g4[i];
            const float2 gb = g5[i];
            const float alpha = al[i];
            const float test_T = T * (1.0f - alpha);
            const bool ok = test_T >= kTMin;
            const float ae = ok ? alpha : 0.0f;
            const float w = ae * T;
            const float A = 1.0f - T, mz = mm[i];
            dist += (mz * mz * A + M2 - 2.0f * mz * M1) * w;
            Dp += dz[i] * w; M1 += mz * w; M2 += mz * mz * w;
            const bool contributes = okv[i] & ok;   // = (ae > 0): a hit that passed eval_surfel has alpha >= 1 / 255 (two scalar masks)
            const bool is_med = contributes & (T > 0.5f);
            med = is_med ? dz[i] : med;
            if constexpr (kForBackward) med_c = is_med ? pos[i] : med_c;
            N0 += nr.x * w; N1 += nr.y * w; N2 += nr.z * w;
            C0 += nr.w * w; C1 += gb.x * w; C2 += gb.y * w;
            T = ok ? test_T : -fabsf(T);
            if constexpr (kForBackward) last = contributes ? pos[i] : last;
          }
        }
      }
      head = head + k2FGroup == k2FRing ? 0 : head + k2FGroup;
      count -= nslots;
    };
    while (count >= k2FGroup) blend_group(std::true_type{}, k2FGroup);
    if (last_chunk && count > 0) blend_group(std::false_type{}, count);
    id0 = id1; r0 = nx0; r1 = nx1; r2 = nx2; r3 = nx3; r4 = nx4; r5 = nx5; id1 = id2;
  }
  if constexpr (kScore) {
#pragma clang fp contract(off)   // divide, the two products, their sum: the roundings of the expression in torch
    float term = 0.0f;
    if (inside) {
      const float a_ = 1.0f - fabsf(T);   // = allmap[1]
      // (the target is ONE hypothesis' stack of views; score_rows is a multiple of the tile, so the block lies in one of them)
      const size_t tp = (size_t)(by % score_rows + (lane >> 3)) * W + px;
      const float e = nan_to_num00(Dp / a_), m = nan_to_num00(med);
      const float sd = e * (1.0f - depth_ratio) + depth_ratio * m;
      term = fabsf(a_ - tgt_alpha[tp]) + fabsf(sd - tgt_depth[tp]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) term += __shfl_xor(term, off, 64);
    if (lane == 0) block_terms[tile * 4 + quad] = term;
    return;
  }
  if (inside) {
    const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
    T = fabsf(T);
    if constexpr (kForBackward) {
      final_T[pix] = T; final_T[HW + pix] = M1; final_T[2 * HW + pix] = M2;
      n_contrib[pix] = last; n_contrib[HW + pix] = med_c;
    }
    out_color[pix] = C0 + T * bg[0]; out_color[HW + pix] = C1 + T * bg[1]; out_color[2 * HW + pix] = C2 + T * bg[2];
    allmap[pix] = Dp; allmap[HW + pix] = 1.0f - T;
    allmap[2 * HW + pix] = N0; allmap[3 * HW + pix] = N1; allmap[4 * HW + pix] = N2;
    allmap[5 * HW + pix] = med; allmap[6 * HW + pix] = dist;
  }
}

// band_h / band_magic of blend2d_forward_wave_kernel for V views of H rows each
struct Bands { int band_h; uint64_t magic; };
Bands bands_of(int V, int H) {
  if (V <= 1) return {0, 0ull};
  const uint64_t d = (uint64_t)(H / kTile);
  return {H, ((1ull << 32) + d - 1) / d};
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_gs2d_state_bytes(int32_t N, int32_t W, int32_t H) { return StateLayout(N, W, H, true).total; }

extern "C" int scorp_gs2d_preprocess(const ScorpGs3dInputs *in, int32_t *out_radii, void *state, size_t state_bytes,
                                     scorp_stream_t stream) {
  return preprocess2d_impl(in, out_radii, state, state_bytes, stream);
}

int scorp::preprocess2d_impl(const ScorpGs3dInputs *in, int32_t *out_radii, void *state, size_t state_bytes, scorp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  return preprocess_pass(kGs2d, in, out_radii, state, state_bytes, stream, [&](const StateLayout &L, char *base) {
    launch_preprocess2d(in, L, (Surfel *)(base + L.rec), (BinRec *)(base + L.bin), (uint64_t *)(base + L.tile_mask), out_radii,
                        (uint32_t *)(base + L.tile_count), stream);
  });
}

int scorp::render2d_impl(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity, float *out_color,
                         float *out_allmap, scorp_stream_t stream_, bool for_backward) {
  hipStream_t stream = (hipStream_t)stream_;
  RenderFrame f;
  if (int e = render_frame(kGs2d, in, state, pairs, capacity, for_backward, &f)) return e;
  if (!out_color || !out_allmap) { set_error("output image pointer is NULL"); return SCORP_ERR_INVALID; }
  const StateLayout &L = f.L;
  if (int e = bin_scatter_and_sort(L, f.P, f.base, f.pb, f.N, f.capacity, in->debug, stream)) return e;
  {
    ProfScope prof(kKBlendForward2d, stream);
    auto bk = for_backward ? blend2d_forward_wave_kernel<true> : blend2d_forward_wave_kernel<false>;
    const Bands b = bands_of(f.V, in->image_height);
    bk<<<block_wave_grid(L.tiles), 64, 0, stream>>>(
        (const uint32_t *)(f.base + L.tile_start), (const uint32_t *)(f.pb + f.P.list), (const Surfel *)(f.base + L.rec),
        f.capacity, f.W, f.H, L.tiles_x, L.tiles, in->bg, out_color, out_allmap, (float *)(f.base + L.final_T),
        (uint32_t *)(f.base + L.n_contrib), (uint32_t *)(f.pb + f.P.hits), b.band_h, b.magic, nullptr, nullptr, 0, 0.0f, nullptr);
  }
  SCORP_KERNEL_CHECK("blend_forward_2d", in->debug, stream);
  return SCORP_OK;
}

// The render-and-compare scoring of pose hypotheses (align.StackedSweep): the argument checks and the band sums of
// scorp_gs3d_render_score, the surface depth of the 2DGS renderer (depth_ratio) in place of depth / alpha.
extern "C" int scorp_gs2d_render_score(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity,
                                       const float *tgt_depth, const float *tgt_alpha, int32_t rows_per_score, float depth_ratio,
                                       float scale, float *acc, scorp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RenderFrame f;
  if (int e = render_frame(kGs2d, in, state, pairs, capacity, false, &f)) return e;
  const int W = f.W, H = f.H;
  if (!tgt_depth || !tgt_alpha || !acc || rows_per_score <= 0 || rows_per_score % kTile != 0 || H % rows_per_score != 0) {
    set_error("scorp_gs2d_render_score: targets / acc NULL, or rows_per_score (%d) not a multiple of 16 dividing the %d rows", rows_per_score, H);
    return SCORP_ERR_INVALID;
  }
  if (!(depth_ratio >= 0.0f && depth_ratio <= 1.0f)) {   // (NaN fails both comparisons)
    set_error("scorp_gs2d_render_score: depth_ratio %g is not in [0, 1]", (double)depth_ratio); return SCORP_ERR_INVALID;
  }
  const StateLayout &L = f.L;
  const int scores = H / rows_per_score, blocks_per_score = (rows_per_score / kTile) * L.tiles_x * 4;
  if (score_bands_too_many(scores, W, H)) { set_error("scorp_gs2d_render_score: too many bands for the image"); return SCORP_ERR_INVALID; }
  if (int e = bin_scatter_and_sort(L, f.P, f.base, f.pb, f.N, f.capacity, in->debug, stream)) return e;
  {
    ProfScope prof(kKBlendForward2d, stream);
    const Bands b = bands_of(f.V, in->image_height);
    float *block_terms = (float *)(f.base + L.block_hits);
    blend2d_forward_wave_kernel<false, true><<<block_wave_grid(L.tiles), 64, 0, stream>>>(
        (const uint32_t *)(f.base + L.tile_start), (const uint32_t *)(f.pb + f.P.list), (const Surfel *)(f.base + L.rec),
        f.capacity, W, H, L.tiles_x, L.tiles, in->bg, nullptr, nullptr, nullptr, nullptr, (uint32_t *)(f.pb + f.P.hits),
        b.band_h, b.magic, tgt_depth, tgt_alpha, rows_per_score, depth_ratio, block_terms);
    // the blocks of score j are the tiles of rows [j, j + 1) * rows_per_score: contiguous tile ids, four blocks each;
    // the partial sums go to the per-pixel state of a backward pass, which this form does not use
    launch_score_bands(block_terms, scores, blocks_per_score, (float *)(f.base + L.final_T), scale, acc, stream);
  }
  SCORP_KERNEL_CHECK("blend_forward_2d_score", in->debug, stream);
  return SCORP_OK;
}

extern "C" int scorp_gs2d_render(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity,
                                 float *out_color, float *out_allmap, scorp_stream_t stream) {
  return render2d_impl(in, state, pairs, capacity, out_color, out_allmap, stream, true);
}

extern "C" int scorp_gs2d_render_image(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity,
                                       float *out_color, float *out_allmap, scorp_stream_t stream) {
  return render2d_impl(in, state, pairs, capacity, out_color, out_allmap, stream, false);
}

// xy[N,2], depth[N], T[N,9], normal_opacity[N,4], rgb[N,3], rect[N,4]; any may be NULL (stage-level parity tests)
extern "C" int scorp_gs2d_debug_geom(const void *state, int32_t N, int32_t W, int32_t H, float *T, float *xy, float *depth,
                                     float *normal_opacity, float *rgb, int32_t *rect, scorp_stream_t stream) {
  void *host;
  const BinRec *hbin;
  if (int e = copy_geom_to_host(state, StateLayout(N, W, H, true), N, sizeof(Surfel), &host, &hbin, (hipStream_t)stream)) return e;
  const Surfel *hrec = (const Surfel *)host;
  for (int i = 0; i < N; i++) {
    const bool vis = (hbin[i].radius & kRadiusMask) != 0;
    const Surfel z = {};
    const Surfel &s = vis ? hrec[i] : z;
    const float t9[9] = {s.r0.x, s.r0.y, s.r0.z, s.r0.w, s.r1.x, s.r1.y, s.r1.z, s.r1.w, s.r2.x};
    if (T) memcpy(T + 9 * (size_t)i, t9, sizeof(t9));
    if (xy) { xy[2 * i] = s.r2.y; xy[2 * i + 1] = s.r2.z; }
    if (depth) { uint32_t b = vis ? hbin[i].depth_bits : 0u; memcpy(depth + i, &b, 4); }
    if (normal_opacity) { normal_opacity[4 * i] = s.r3.x; normal_opacity[4 * i + 1] = s.r3.y; normal_opacity[4 * i + 2] = s.r3.z; normal_opacity[4 * i + 3] = s.r2.w; }
    if (rgb) { rgb[3 * i] = s.r3.w; rgb[3 * i + 1] = s.r4.x; rgb[3 * i + 2] = s.r4.y; }
    if (rect) { rect[4 * i] = vis ? hbin[i].x0 : 0; rect[4 * i + 1] = vis ? hbin[i].y0 : 0; rect[4 * i + 2] = vis ? hbin[i].x1 : 0; rect[4 * i + 3] = vis ? hbin[i].y1 : 0; }
  }
  free(host);
  return SCORP_OK;
}

extern "C" int scorp_gs2d_debug_tiles(const void *state, const void *pairs, uint64_t capacity, int32_t N, int32_t W,
                                      int32_t H, uint32_t *tile_start, uint32_t *point_list, scorp_stream_t stream) {
  return debug_tiles(true, state, pairs, capacity, N, W, H, tile_start, point_list, (hipStream_t)stream);
}
