// gs3d_forward.hip — 3DGS forward for gfx950: project (gs3d_pergaussian.hip) -> bin and depth-sort the (tile, splat)
// pairs (binning.hip) -> front-to-back blend; and the render-and-compare scoring of the pose sweep.
//
// Replaces the forward half of `diff_gaussian_rasterization` as called at
// gs3dgs/gaussian_renderer/__init__.py:101-111.  The arithmetic follows oracle/gs3d_oracle.c (the CPU
// restatement of the published algorithm).
#include <stdlib.h>

#include <type_traits>

#include "common.hpp"
#include "exp_mfma.hpp"

namespace scorp {
namespace {

// ---------------------------------------------------------------------------------------------------------
// K5: front-to-back blend with ONE WAVE PER 8x8 BLOCK as the unit (64-thread workgroups, no workgroup barriers), the
// forward twin of blend_backward_wave_kernel: the wave walks the tile's list front to back 64 entries at a time, each
// lane gathers one record and runs the exact conic-vs-block test, survivors are compacted into a per-wave LDS ring,
// and groups of 8 go through a straight-line alpha phase followed by the branch-free sequential blend (a splat that
// does not contribute to a pixel enters as alpha = 0, which changes nothing).  Stops as soon as all 64 pixels are
// saturated.  The four waves of a tile are numbered onto the same XCD.
// For the backward it leaves the block's HIT LIST (the splat ids that passed the test, in list order, compacted, in the
// dead key region of the pair buffer) and per pixel the final T and the 1-based position IN THAT LIST of the last splat
// that contributed: the backward replays the hit list and never looks at the tile's list again.
// ---------------------------------------------------------------------------------------------------------
// The exponent log2(opacity * G) of a group of 16 hits at the block's 64 pixels comes from the matrix cores (exp_mfma.hpp:
// three v_mfma_f32_32x32x16_bf16 against the lane's own monomials; register i of a lane = splat i at that lane's pixel):
// the lane that stages a hit turns its record into the six block-frame coefficients, cut into three bf16 terms each, and a
// ring slot holds those 48 bytes plus (r, g, b, depth).  The sequential blend then costs, per hit and pixel: v_exp, the
// two threshold selects, the T update and four accumulations - the seven VALU instructions of the Horner form (35 % of the
// old loop's issue time together with its LDS reads of the conic) are gone.  A hit's 1-based position in the block's hit
// list is arithmetic (hits are blended in ring order): no position array.
#ifndef SCORP_FWD_RING
#define SCORP_FWD_RING 80
#endif
constexpr int kFRing = SCORP_FWD_RING, kFChunk = 64, kFGroup = 16;   // ring: at most 15 left-over hits + 64 new ones

// __launch_bounds__(64, 6): six waves per SIMD = at most 80 registers.  The kernel needs 84 - 86 left to itself since it
// compacts the hit list (round 4); held to 80 it spills ONE register outside the per-hit loop and keeps its sixth wave
// (same box, rocprof: 157.4 us at five waves per SIMD, 153.4 at six; 148.7 before the compaction, which takes 22 us off
// the backward).  The MFMA results stay in VGPRs either way (no accumulator-register reads in front of the v_exp).
#ifndef SCORP_FWD_WAVES
#define SCORP_FWD_WAVES 6
#endif
// kScore (scorp_gs3d_render_score; never with kForBackward): the render-and-compare scoring of a pose hypothesis
// (align.StackedSweep) needs depth and alpha only and needs them only to be compared with a target: no colour is
// accumulated (three of the hit loop's thirteen vector instructions), no image is written, and the epilogue forms this
// pixel's |alpha - alpha*| + |nan_to_num(depth / alpha) - depth*| (scorp_gs3d_pose_score_accumulate's term), sums it over
// the block and leaves ONE float per block in the state's block_hits array - plain stores, added up in a fixed order by
// score_reduce_kernel (so the score, unlike the atomic form's, is the same bits from run to run).
template <bool kForBackward, bool kScore = false>
__global__ void __launch_bounds__(64, SCORP_FWD_WAVES)
blend_forward_wave_kernel(const uint32_t *__restrict__ tile_start, const uint32_t *__restrict__ point_list,
                          const SplatRec *__restrict__ rec, uint32_t capacity, int W, int H, int tiles_x, int tiles,
                          const float *__restrict__ bg, float *__restrict__ out_color, float *__restrict__ out_depth,
                          float *__restrict__ out_alpha, float *__restrict__ final_T, uint32_t *__restrict__ n_contrib,
                          uint32_t *__restrict__ hits, uint32_t *__restrict__ block_hits, float *__restrict__ out_depth_norm,
                          float4 *__restrict__ zero_buf, uint32_t zero_per_wave, uint32_t zero_total, int band_h,
                          const float *__restrict__ tgt_depth = nullptr, const float *__restrict__ tgt_alpha = nullptr,
                          int score_rows = 0) {
  static_assert(!(kForBackward && kScore), "the scoring form leaves nothing behind for a backward pass");
  __shared__ uint4 q_k[3][kFRing + 1];   // the three bf16 terms of a hit's six coefficients; slot kFRing stays zero
  __shared__ float4 q_col[kFRing];       // r, g, b, depth
  __shared__ uint32_t q_id[kFRing];      // the hit's splat: written to the block's hit list only if some pixel took it (blend_group)
  const int lane = threadIdx.x;
  if (zero_buf) {   // this wave's share of the buffer the launch was asked to clear (every workgroup of the grid takes part)
    const uint32_t z0 = blockIdx.x * zero_per_wave, z1 = min(z0 + zero_per_wave, zero_total);
    typedef float f4v __attribute__((ext_vector_type(4)));
    const f4v zero = {0.0f, 0.0f, 0.0f, 0.0f};   // streaming stores: the rows are not read before the backward, keep them out of L2
    for (uint32_t z = z0 + lane; z < z1; z += 64) __builtin_nontemporal_store(zero, reinterpret_cast<f4v *>(zero_buf) + z);
  }
  BlockWave blk;
  if (!block_wave(tiles, tiles_x, blk)) return;
  const int tile = blk.tile, quad = blk.quad, bx = blk.bx, by = blk.by;
  const int px = bx + (lane & 7), py = by + (lane >> 3);
  const bool inside = px < W && py < H;
  // stacked views (ScorpGs3dInputs.num_views): the records hold each view's OWN pixel coordinates, so the block's frame
  // is taken relative to the first row of its band (band_h = rows per view, 0 = one view)
  const int byl = band_h > 0 ? by % band_h : by;
  const float bx0 = (float)bx, bx1 = (float)(bx + 7), by0 = (float)byl, by1 = (float)(byl + 7);
  const float cx = (float)bx + 3.5f, cy = (float)byl + 3.5f;
  const TileRange tr = tile_range(tile_start, tile, capacity);
  const uint32_t beg = tr.beg, n = tr.end - tr.beg;
  uint32_t *my_hits = block_hit_list(hits, quad, capacity, beg);
  if (lane < 3) q_k[lane][kFRing] = make_uint4(0u, 0u, 0u, 0u);
  const uint4 basis = pixel_basis_frag(lane);
  const bool a_on = a_operand_active(lane);
  const int a_slot = a_operand_slot(lane);
  float T = inside ? 1.0f : -1.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, Dp = 0.0f;   // T < 0: pixel finished (see below)
  uint32_t last = 0;
  int head = 0, count = 0;   // head stays a multiple of kFGroup (only a wave's final group is partial), so the
                             // slots of a group are head + i without wrap-around: one LDS base, immediate offsets
  uint32_t nh = 0;           // hits found so far (wave-uniform)
  uint32_t consumed = 0;     // hits blended so far ((block, splat) iterations: the P statistic)
  uint32_t kept_n = 0;       // ... of which some pixel took: the length of the hit list left for the backward (wave-uniform)
  uint32_t hot_end = 0;      // hits [0, hot_end) may hold a splat with opacity > 0.99 (wave-uniform; see blend_group)
  // The chunk's gathers (list entry -> record) are dependent loads of ~1 us each; they are software-pipelined: while
  // chunk c is blended the records of chunk c+1 and the list entries of chunk c+2 are already in flight.
  auto fetch_id = [&](uint32_t bs) { return (bs + lane < n) ? point_list[beg + bs + lane] : 0xFFFFFFFFu; };
  auto fetch_rec = [&](uint32_t id_, float4 &a_, float4 &b_, float4 &c_) {
    if (id_ != 0xFFFFFFFFu) {
      const float4 *src = reinterpret_cast<const float4 *>(rec + id_);
      a_ = src[0]; b_ = src[1]; c_ = src[2];
    }
  };
  float4 a, b, c;
  uint32_t id0 = fetch_id(0);
  fetch_rec(id0, a, b, c);
  uint32_t id1 = fetch_id(kFChunk);
  for (uint32_t base = 0; base < n; base += kFChunk) {
    if (__ballot(T > 0.0f) == 0) break;
    float4 a1, b1, c1;
    fetch_rec(id1, a1, b1, c1);
    const uint32_t id2 = fetch_id(base + 2 * kFChunk);
    bool hit = false;
    if (id0 != 0xFFFFFFFFu)   // the record holds -k * conic and k * cutoff (k > 0): the test is scale-invariant
      hit = rec_is_indefinite(c.z) || conic_min_over_box(a.x, a.y, -a.z, -0.5f * a.w, -b.x, bx0, bx1, by0, by1) <= c.z;
    const uint64_t m = __ballot(hit);
    if (hit) {
      const uint32_t rank = nh + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
      int qi = head + count + (int)(rank - nh);
      qi = qi >= kFRing ? qi - kFRing : qi;
      uint4 k0, k1, k2;
      splat_block_coefs(a.x, a.y, a.z, a.w, b.x, b.y, cx, cy, k0, k1, k2);
      k0.w = guard_limit_pack(c.w);   // (spare K slots: exp_mfma.hpp)
      q_k[0][qi] = k0; q_k[1][qi] = k1; q_k[2][qi] = k2;
      q_col[qi] = make_float4(b.z, b.w, c.x, c.y);
      if constexpr (kForBackward) q_id[qi] = id0;
    }
    count += __builtin_popcountll(m);
    nh += (uint32_t)__builtin_popcountll(m);
    // (b.y = log2(opacity); the margin keeps exp2(e) <= 0.99 for every other hit whatever the rounding of e)
    // ... and an indefinite conic needs the `power > 0` guard, which the same instantiation carries
    if (__ballot(hit && (b.y > kLog2AlphaMax - 1e-4f || rec_is_indefinite(c.z))) != 0) hot_end = nh;   // groups up to this chunk's last hit keep the clamp
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const bool last_chunk = base + kFChunk >= n;
    // full groups run straight-line (nslots is the compile-time kFGroup); only a wave's final group is partial
    // log2(opacity * G) of the 16 hits in ring slots h .. h + 15 at this lane's pixel (three MFMAs)
    auto exponents = [&](int h) -> f32x16 {
      int hv = h;
      asm volatile("" : "+v"(hv));
      const int sl = a_on ? hv + a_slot : kFRing;      // the other half of the lanes feeds zeros (exp_mfma.hpp)
      return block_exponents(q_k[0][sl], q_k[1][sl], q_k[2][sl], basis);
    };
    auto blend_group = [&](auto full, auto clampy, int nslots, const f32x16 &e) -> bool {
      constexpr bool kFull = decltype(full)::value;
      // alpha = min(0.99, opacity * G) and G <= 1: the clamp can only bind for a splat whose opacity itself exceeds 0.99.
      // Groups that hold no such hit (all but a few per cent on any scene: opacity > 0.99 is sigmoid(x), x > 4.6) run
      // without the v_min - one VALU instruction of the fourteen per hit.
      constexpr bool kClamp = decltype(clampy)::value;
      int hv = head;
      asm volatile("" : "+v"(hv));   // keep the group's LDS bases in VGPRs (else every ds_read re-moves an SGPR base)
      const float4 *gc = q_col + hv;
      const uint4 *gk = q_k[0] + hv;
      bool all_done = false;
      uint32_t lastg = 0;   // 1-based slot of the group's last contributor to this pixel (inline constants, no SGPR moves)
      uint32_t kept16 = 0;  // wave-uniform: bit i = slot i was taken by at least one pixel of the block
#pragma unroll
      for (int i = 0; i < kFGroup; i++) {
        if (kFull || i < nslots) {  // wave-uniform
          if (kFull && i == kFGroup / 2) {   // every pixel saturated already: the second half is not needed
            if (__ballot(T > 0.0f) == 0) { all_done = true; break; }
          }
          const float4 col = gc[i];
          const float g_o = __builtin_amdgcn_exp2f(e[i]);
          const float alpha = kClamp ? fminf(kAlphaMax, g_o) : g_o;
          bool live = alpha >= kAlphaMin;
          if constexpr (kClamp) live = live & (g_o <= guard_limit_unpack(gk[i].w));   // the reference's `power > 0` skip (exp_mfma.hpp)
          const float al = live ? alpha : 0.0f;
          // A saturated pixel is latched by the SIGN of T: the splat that would take T below 1e-4 is not blended and
          // flips T negative, after which every test_T is negative too (a live pixel always has T >= 1e-4, and
          // alpha = 0 leaves test_T = T exactly).
          const float test_T = __builtin_fmaf(-al, T, T);
          const bool ok = test_T >= kTMin;
          const float ae = ok ? al : 0.0f;
          const float w = ae * T;
          if constexpr (!kScore) { C0 += col.x * w; C1 += col.y * w; C2 += col.z * w; }
          Dp += col.w * w;
          T = ok ? test_T : -fabsf(T);
          if constexpr (kForBackward) {
            const bool took = ok & live;
            lastg = took ? (uint32_t)(i + 1) : lastg;
            // (each ballot of a plain compare IS that compare's lane mask, and the AND of two 64-bit scalars is scalar work; the
            // ballot of `took` itself - an AND of two conditions - goes through a VGPR 0 / 1 and a second v_cmp: +2 VALU per hit)
            kept16 |= ((__builtin_amdgcn_ballot_w64(ok) & __builtin_amdgcn_ballot_w64(live)) != 0ull ? 1u : 0u) << i;
          }
        }
      }
      if constexpr (kForBackward) {
        // The block's HIT LIST keeps only the hits some pixel took.  A hit passes the exact block test when the conic's
        // minimum over the 8x8 box is below the cutoff - a minimum that may lie between pixel centres, or behind pixels that
        // are already saturated: 6.6 % of the hits of an S3 view have no taker (profiles/r05_lane_occupancy_stats.txt), and the
        // backward, which replays the list, would run its whole per-hit pipeline (and an atomic row of zeros' worth of
        // bookkeeping) for each.  Positions are those of the compacted list: kept hits before this group + rank in it.
        if (lastg) last = kept_n + (uint32_t)__builtin_popcount(kept16 & ((1u << lastg) - 1u));
        if (lane < nslots && ((kept16 >> lane) & 1u))   // (v_mbcnt: the kept slots below this lane's, no lane mask held in a register)
          my_hits[kept_n + __builtin_amdgcn_mbcnt_lo(kept16, 0u)] = q_id[hv + lane];
        kept_n += (uint32_t)__builtin_popcount(kept16);
        __builtin_amdgcn_sched_barrier(0);   // (keeps this tail out of the next group's exponent MFMAs: their sixteen results and
                                             // the tail's temporaries together cost the sixth wave per SIMD)
      }
      head = head + kFGroup == kFRing ? 0 : head + kFGroup;
      count -= nslots;
      consumed += (uint32_t)nslots;
      return all_done;
    };
    bool all_done = false;   // every pixel saturated: checked twice per group, not only once per 64 list entries
    while (count >= kFGroup) {
      const f32x16 e = exponents(head);
      const bool gd = consumed < hot_end ? blend_group(std::true_type{}, std::true_type{}, kFGroup, e)
                                         : blend_group(std::true_type{}, std::false_type{}, kFGroup, e);
      if (gd || __ballot(T > 0.0f) == 0) { all_done = true; break; }
    }
    if (all_done) break;
    if (last_chunk && count > 0) blend_group(std::false_type{}, std::true_type{}, count, exponents(head));   // (one group per wave: not worth a variant)
    id0 = id1; a = a1; b = b1; c = c1; id1 = id2;
  }
  if constexpr (kForBackward) {
    if (lane == 0) block_hits[tile * 4 + quad] = consumed;   // (block, splat) iterations this wave ran: the P statistic
  }
  if constexpr (kScore) {
    float term = 0.0f;
    if (inside) {
      const float a_ = 1.0f - fabsf(T);
      const size_t tp = (size_t)(py % score_rows) * W + px;     // (the target is ONE hypothesis' stack of views)
      term = fabsf(a_ - tgt_alpha[tp]) + fabsf(nan_to_num00(Dp / a_) - tgt_depth[tp]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) term += __shfl_xor(term, off, 64);
    if (lane == 0) reinterpret_cast<float *>(block_hits)[tile * 4 + quad] = term;
    return;
  }
  if (inside) {
    const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
    T = fabsf(T);
    if constexpr (kForBackward) {
      final_T[pix] = T;
      n_contrib[pix] = last;
    }
    out_color[pix] = C0 + T * bg[0];
    out_color[HW + pix] = C1 + T * bg[1];
    out_color[2 * HW + pix] = C2 + T * bg[2];
    out_depth[pix] = Dp;
    out_alpha[pix] = 1.0f - T;   // = sum of the blend weights (sum_i alpha_i T_i telescopes to 1 - T)
    if (out_depth_norm) out_depth_norm[pix] = nan_to_num00(Dp / (1.0f - T));   // render()'s depth, as render_tail_kernel forms it
  }
}

// acc[j] += scale * (the per-block terms of band j), added in a FIXED order and without atomics, in two small launches
// (a band of the sweep holds 150 000 terms: one workgroup walking them is a chain of 600 dependent round trips, ~100 us):
// kScoreSlices workgroups per band each sum a contiguous slice into partial[band][slice], then one workgroup per band adds
// its kScoreSlices partial sums.
constexpr int kScoreSlices = 128;
__device__ __forceinline__ float block_sum_256(float sum, float *s_part) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
  __syncthreads();
  return (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
}
__global__ void __launch_bounds__(256)
score_slices_kernel(const float *__restrict__ block_terms, int blocks_per_score, float *__restrict__ partial) {
  __shared__ float s_part[4];
  const int band = blockIdx.x / kScoreSlices, slice = blockIdx.x % kScoreSlices;
  const int per = (blocks_per_score + kScoreSlices - 1) / kScoreSlices;
  const int i0 = slice * per, i1 = min(i0 + per, blocks_per_score);
  const float *src = block_terms + (size_t)band * blocks_per_score;
  float sum = 0.0f;
  for (int i = i0 + (int)threadIdx.x; i < i1; i += 256) sum += src[i];
  const float tot = block_sum_256(sum, s_part);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}
__global__ void __launch_bounds__(256)
score_reduce_kernel(const float *__restrict__ partial, float scale, float *__restrict__ acc) {
  __shared__ float s_part[4];
  const float tot = block_sum_256(threadIdx.x < kScoreSlices ? partial[blockIdx.x * kScoreSlices + threadIdx.x] : 0.0f, s_part);
  if (threadIdx.x == 0) acc[blockIdx.x] += scale * tot;
}

}  // namespace

bool score_bands_too_many(int scores, int W, int H) { return (size_t)scores * kScoreSlices > (size_t)W * H; }

void launch_score_bands(const float *block_terms, int scores, int blocks_per_score, float *partial, float scale, float *acc,
                        hipStream_t stream) {
  score_slices_kernel<<<scores * kScoreSlices, 256, 0, stream>>>(block_terms, blocks_per_score, partial);
  score_reduce_kernel<<<scores, 256, 0, stream>>>(partial, scale, acc);
}
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_gs3d_state_bytes(int32_t N, int32_t W, int32_t H) { return StateLayout(N, W, H).total; }
extern "C" size_t scorp_gs3d_pairs_bytes(uint64_t capacity) { return PairLayout(capacity).total; }

extern "C" int scorp_gs3d_preprocess(const ScorpGs3dInputs *in, int32_t *out_radii, void *state, size_t state_bytes,
                                     scorp_stream_t stream) {
  return preprocess3d_impl(in, out_radii, nullptr, state, state_bytes, stream);
}

int scorp::preprocess3d_impl(const ScorpGs3dInputs *in, int32_t *out_radii, uint8_t *out_visible, void *state,
                             size_t state_bytes, scorp_stream_t stream_, float *jac) {
  hipStream_t stream = (hipStream_t)stream_;
  return preprocess_pass(kGs3d, in, out_radii, state, state_bytes, stream, [&](const StateLayout &L, char *base) {
    launch_preprocess(in, L, (SplatRec *)(base + L.rec), (BinRec *)(base + L.bin), (uint64_t *)(base + L.tile_mask), out_radii,
                      (uint32_t *)(base + L.tile_count), out_visible, stream, jac);
  });
}

extern "C" int scorp_gs3d_num_pairs(const void *state, scorp_stream_t stream, uint64_t *num_pairs) {
  if (!state || !num_pairs) { set_error("state / num_pairs is NULL"); return SCORP_ERR_INVALID; }
  StateHeader h;
  if (int e = read_header(state, (hipStream_t)stream, &h)) return e;
  *num_pairs = h.num_pairs;
  return SCORP_OK;
}

extern "C" int scorp_gs3d_check_overflow(const void *state, scorp_stream_t stream, uint64_t *num_pairs) {
  if (!state) { set_error("state is NULL"); return SCORP_ERR_INVALID; }
  StateHeader h;
  if (int e = read_header(state, (hipStream_t)stream, &h)) return e;
  if (num_pairs) *num_pairs = h.num_pairs;
  if (h.overflow) {
    set_error("pair buffer overflow: %u pairs needed, capacity %u", h.num_pairs, h.capacity);
    return SCORP_ERR_OVERFLOW;
  }
  return SCORP_OK;
}

int scorp::render3d_impl(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity, float *out_color,
                         float *out_depth, float *out_alpha, float *out_depth_norm, void *zero_buf, size_t zero_bytes,
                         scorp_stream_t stream_, bool for_backward, uint32_t *header_copy) {
  hipStream_t stream = (hipStream_t)stream_;
  RenderFrame f;
  if (int e = render_frame(kGs3d, in, state, pairs, capacity, for_backward, &f)) return e;
  if (!out_color || !out_depth || !out_alpha) { set_error("output image pointer is NULL"); return SCORP_ERR_INVALID; }
  const StateLayout &L = f.L;
  if (int e = bin_scatter_and_sort(L, f.P, f.base, f.pb, f.N, f.capacity, in->debug, stream, header_copy)) return e;
  {
    ProfScope prof(kKBlendForward, stream);
    const int blocks = block_wave_grid(L.tiles);
    const size_t zero_total = zero_buf ? zero_bytes / 16 : 0, zero_per_wave = (zero_total + blocks - 1) / blocks;
    if (zero_buf && (((uintptr_t)zero_buf & 15) || (zero_bytes & 15) || zero_total > 0xFFFFFFFFull)) {
      set_error("render3d_impl: zero_buf must be 16-byte aligned, a multiple of 16 bytes, below 64 GiB"); return SCORP_ERR_INVALID;
    }
    auto bk = for_backward ? blend_forward_wave_kernel<true> : blend_forward_wave_kernel<false>;
    bk<<<blocks, 64, 0, stream>>>(
        (const uint32_t *)(f.base + L.tile_start), (const uint32_t *)(f.pb + f.P.list), (const SplatRec *)(f.base + L.rec),
        f.capacity, f.W, f.H, L.tiles_x, L.tiles, in->bg, out_color, out_depth, out_alpha, (float *)(f.base + L.final_T),
        (uint32_t *)(f.base + L.n_contrib), (uint32_t *)(f.pb + f.P.hits), (uint32_t *)(f.base + L.block_hits), out_depth_norm,
        (float4 *)zero_buf, (uint32_t)zero_per_wave, (uint32_t)zero_total, f.V > 1 ? in->image_height : 0, nullptr, nullptr, 0);
  }
  SCORP_KERNEL_CHECK("blend_forward", in->debug, stream);
  return SCORP_OK;
}

extern "C" int scorp_gs3d_render(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity,
                                 float *out_color, float *out_depth, float *out_alpha, scorp_stream_t stream) {
  return render3d_impl(in, state, pairs, capacity, out_color, out_depth, out_alpha, nullptr, nullptr, 0, stream, true);
}

extern "C" int scorp_gs3d_render_image(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity,
                                       float *out_color, float *out_depth, float *out_alpha, scorp_stream_t stream) {
  return render3d_impl(in, state, pairs, capacity, out_color, out_depth, out_alpha, nullptr, nullptr, 0, stream, false);
}

extern "C" int scorp_gs3d_render_score(const ScorpGs3dInputs *in, void *state, void *pairs, uint64_t capacity,
                                       const float *tgt_depth, const float *tgt_alpha, int32_t rows_per_score, float scale,
                                       float *acc, scorp_stream_t stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  RenderFrame f;
  if (int e = render_frame(kGs3d, in, state, pairs, capacity, false, &f)) return e;
  const int W = f.W, H = f.H;
  if (!tgt_depth || !tgt_alpha || !acc || rows_per_score <= 0 || rows_per_score % kTile != 0 || H % rows_per_score != 0) {
    set_error("scorp_gs3d_render_score: targets / acc NULL, or rows_per_score (%d) not a multiple of 16 dividing the %d rows", rows_per_score, H);
    return SCORP_ERR_INVALID;
  }
  const StateLayout &L = f.L;
  char *base = f.base;
  if (int e = bin_scatter_and_sort(L, f.P, base, f.pb, f.N, f.capacity, in->debug, stream, nullptr)) return e;
  {
    ProfScope prof(kKBlendForward, stream);
    const int blocks = block_wave_grid(L.tiles);
    blend_forward_wave_kernel<false, true><<<blocks, 64, 0, stream>>>(
        (const uint32_t *)(base + L.tile_start), (const uint32_t *)(f.pb + f.P.list), (const SplatRec *)(base + L.rec), f.capacity,
        W, H, L.tiles_x, L.tiles, in->bg, nullptr, nullptr, nullptr, nullptr, nullptr, (uint32_t *)(f.pb + f.P.hits),
        (uint32_t *)(base + L.block_hits), nullptr, nullptr, 0u, 0u, f.V > 1 ? in->image_height : 0, tgt_depth, tgt_alpha,
        rows_per_score);
    // the blocks of score j are the tiles of rows [j, j + 1) * rows_per_score: contiguous tile ids, four blocks each
    const int scores = H / rows_per_score, blocks_per_score = (rows_per_score / kTile) * L.tiles_x * 4;
    float *partial = (float *)(base + L.final_T);   // (the per-pixel state of a backward pass: unused by this form)
    if (score_bands_too_many(scores, W, H)) { set_error("scorp_gs3d_render_score: too many bands for the image"); return SCORP_ERR_INVALID; }
    launch_score_bands((const float *)(base + L.block_hits), scores, blocks_per_score, partial, scale, acc, stream);
  }
  SCORP_KERNEL_CHECK("blend_forward_score", in->debug, stream);
  return SCORP_OK;
}

extern "C" int scorp_gs3d_debug_geom(const void *state, int32_t N, int32_t W, int32_t H, float *xy, float *depth,
                                     float *conic_opacity, float *rgb, int32_t *rect, scorp_stream_t stream) {
  void *host;
  const BinRec *hbin;
  if (int e = copy_geom_to_host(state, StateLayout(N, W, H), N, sizeof(SplatRec), &host, &hbin, (hipStream_t)stream)) return e;
  const SplatRec *hrec = (const SplatRec *)host;
  for (int i = 0; i < N; i++) {
    const bool vis = (hbin[i].radius & kRadiusMask) != 0;
    const SplatRec z = {};
    const SplatRec &s = vis ? hrec[i] : z;
    if (xy) { xy[2 * i] = s.x; xy[2 * i + 1] = s.y; }
    if (depth) depth[i] = s.depth;
    if (conic_opacity) {   // back from the exponent form
      conic_opacity[4 * i] = s.A * (-1.0f / kConicScale); conic_opacity[4 * i + 1] = s.B * (-0.5f / kConicScale);
      conic_opacity[4 * i + 2] = s.C * (-1.0f / kConicScale); conic_opacity[4 * i + 3] = s.o;
    }
    if (rgb) { rgb[3 * i] = s.r; rgb[3 * i + 1] = s.g; rgb[3 * i + 2] = s.b; }
    if (rect) { rect[4 * i] = vis ? hbin[i].x0 : 0; rect[4 * i + 1] = vis ? hbin[i].y0 : 0; rect[4 * i + 2] = vis ? hbin[i].x1 : 0; rect[4 * i + 3] = vis ? hbin[i].y1 : 0; }
  }
  free(host);
  return SCORP_OK;
}

extern "C" int scorp_gs3d_debug_work(const void *state, int32_t N, int32_t W, int32_t H, uint64_t *out3, scorp_stream_t stream_) {
  if (!state || !out3) { set_error("NULL argument to scorp_gs3d_debug_work"); return SCORP_ERR_INVALID; }
  hipStream_t stream = (hipStream_t)stream_;
  const StateLayout L(N, W, H);
  const size_t nb = (size_t)L.tiles * 4, hw = (size_t)W * H;
  uint32_t *hb = (uint32_t *)malloc(nb * 4), *hc = (uint32_t *)malloc(hw * 4);
  if (!hb || !hc) { free(hb); free(hc); set_error("host allocation failed"); return SCORP_ERR_INVALID; }
  hipError_t e = hipMemcpyAsync(hb, (const char *)state + L.block_hits, nb * 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipMemcpyAsync(hc, (const char *)state + L.n_contrib, hw * 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { free(hb); free(hc); set_error("debug_work copy failed: %s", hipGetErrorString(e)); return SCORP_ERR_HIP; }
  uint64_t fwd = 0, bwd = 0;
  for (size_t b = 0; b < nb; b++) fwd += hb[b];
  const int tiles_x = L.tiles_x;
  for (int t = 0; t < L.tiles; t++)
    for (int q = 0; q < 4; q++) {   // the backward replays, per block, up to the deepest last contributor of its pixels
      const int bx = (t % tiles_x) * kTile + (q & 1) * 8, by = (t / tiles_x) * kTile + (q >> 1) * 8;
      uint32_t m = 0;
      for (int y = by; y < by + 8 && y < H; y++)
        for (int x = bx; x < bx + 8 && x < W; x++) m = hc[(size_t)y * W + x] > m ? hc[(size_t)y * W + x] : m;
      bwd += m;
    }
  out3[0] = fwd; out3[1] = bwd; out3[2] = (uint64_t)nb;
  free(hb); free(hc);
  return SCORP_OK;
}

extern "C" int scorp_gs3d_debug_tiles(const void *state, const void *pairs, uint64_t capacity, int32_t N, int32_t W,
                                      int32_t H, uint32_t *tile_start, uint32_t *point_list, scorp_stream_t stream) {
  return debug_tiles(false, state, pairs, capacity, N, W, H, tile_start, point_list, (hipStream_t)stream);
}

// What the blend forward left behind for the backward and the vote, copied out as it stands (no kernel, nothing written on
// the device): the hit lists re-addressed from the pair buffer's order into the raster tile order of debug_tiles.
extern "C" int scorp_gs3d_debug_blend(const void *state, const void *pairs, uint64_t capacity, int32_t N, int32_t W, int32_t H,
                                      float *final_T, uint32_t *n_contrib, uint32_t *block_hits, uint32_t *out_hits,
                                      scorp_stream_t stream_) {
  if (W <= 0 || H <= 0 || N < 0) { set_error("scorp_gs3d_debug_blend: N (%d) negative or W x H (%d x %d) empty", N, W, H); return SCORP_ERR_INVALID; }
  if (int e = check_buffers(state, pairs, capacity)) return e;
  hipStream_t stream = (hipStream_t)stream_;
  const StateLayout L(N, W, H);
  const PairLayout P(capacity);
  StateHeader h;
  if (int e = read_header(state, stream, &h)) return e;
  const size_t n = h.num_pairs < capacity ? h.num_pairs : (size_t)capacity, hw = (size_t)W * H, nb = (size_t)L.tiles * 4;
  const bool lists = out_hits && n > 0;
  uint32_t *range = lists ? (uint32_t *)malloc((size_t)L.tiles * 8) : nullptr, *raw = lists ? (uint32_t *)malloc(n * 16) : nullptr;
  if (lists && (!range || !raw)) { free(range); free(raw); set_error("host allocation failed"); return SCORP_ERR_INVALID; }
  const char *sb = (const char *)state, *pb = (const char *)pairs;
  hipError_t e = hipSuccess;
  if (final_T) e = hipMemcpyAsync(final_T, sb + L.final_T, hw * 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && n_contrib) e = hipMemcpyAsync(n_contrib, sb + L.n_contrib, hw * 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && block_hits) e = hipMemcpyAsync(block_hits, sb + L.block_hits, nb * 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess && lists) e = hipMemcpyAsync(range, sb + L.tile_start, (size_t)L.tiles * 8, hipMemcpyDeviceToHost, stream);
  for (int q = 0; q < 4 && e == hipSuccess && lists; q++)   // hits[quad][capacity]: the first n entries of each region
    e = hipMemcpyAsync(raw + (size_t)q * n, pb + P.hits + (size_t)q * capacity * 4, n * 4, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) { free(range); free(raw); set_error("debug_blend copy failed: %s", hipGetErrorString(e)); return SCORP_ERR_HIP; }
  if (lists) {
    size_t run = 0;
    for (int t = 0; t < L.tiles; t++) {   // (the ranges clamped as debug_tiles clamps them: the same tile_start)
      const size_t b = range[2 * t] < n ? range[2 * t] : n, en = range[2 * t + 1] < n ? range[2 * t + 1] : n;
      if (en > b) {
        for (int q = 0; q < 4; q++) memcpy(out_hits + (size_t)q * n + run, raw + (size_t)q * n + b, (en - b) * 4);
        run += en - b;
      }
    }
  }
  free(range); free(raw);
  return SCORP_OK;
}
