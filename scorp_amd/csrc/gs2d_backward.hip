// gs2d_backward.hip — 2D Gaussian splatting (surfel) path for gfx950: the blend backward (one wave per 8x8 pixel block,
// replaying the hit list the forward of gs2d_forward.hip left; the pixel -> surfel reduction on the matrix cores) and the
// backward entry points.  The per-surfel kernel that turns its accumulators into gradients is in gs2d_pergaussian.hip.
#include "surfel.hpp"

namespace scorp {
namespace {

// ---------------------------------------------------------------------------------------------------------
// The pixel -> surfel reduction of the 2-D backward on the matrix cores (round 4; it was a twenty-value butterfly of
// v_permlane32 / 16_swap + DPP adds: 15 swaps at 8.4 issue cycles + 27 adds per hit, 44 % of the kernel).
//
// The twenty sums of a hit factor, like the ten of the 3-D kernel, into a handful of per-pixel VALUES times per-pixel
// BASES that do not depend on the hit:
//     dp0, dp1, dp2  x {x, y, 1}                (nine sums: d/d pa, pb, pc; x, y = the pixel about the block centre - the offset to
//                                                the surfel's accumulation point is a per-hit constant applied afterwards)
//     zr, z2, t x {1};   t2 x {x, y, 1}         (depth, low-pass depth, opacity; the low-pass centre gradient)
//     w x {dL/dn (3), dL/drgb (3)}              (normal and colour)
// Eight values per (hit, pixel).  Each leaves the lane as TWO fp16 terms (x = h1 + h2, h1 = rtz16(x), h2 = rtz16(x - h1):
// 22 bits, exact products, fp32 accumulation), both in ONE dword, so a hit costs eight ds_write_b32; rows of the matrix
// are (hit of the pair, kind), its K dimension (pixel, term); B holds each basis value twice (once per term: the MFMA
// adds the two terms by itself) - columns 0 = 1, 1 = x, 2 = y, 3..8 = the first fp16 term of the six upstream gradients,
// 9..14 = their remainder.  Two hits per pass, four v_mfma_f32_16x16x32_f16 per pass.
// Range: block floating point, three exact powers of two.  The upstream gradients are pre-scaled per wave from the
// block's largest |dL/dpixel| (everything the recurrence produces is linear in them: the B operand's gradient columns
// sit high in the fp16 range); the four values that contain 1 / p.z (p.z ~ surfel extent^2 in pixels: anything from 1e-3
// to 1e3) are scaled per hit by the power of two below |p.z| at the block centre; and the three per-pixel roots of a
// hit - all eight values are linear in them - by the power of two that brings the largest of them over the hit's pixels
// into [2^4, 2^5) (one wave maximum per hit), so that the pair's 22 bits hold down to 2^-17 of the hit's largest value
// whatever T, alpha and the depth scale are.  The blend weight is carried as w * 2^10.  The conversion saturates
// (round toward zero) instead of overflowing.  The sums are unscaled by exact powers of two when they are read out.
// ---------------------------------------------------------------------------------------------------------
typedef float f32x4_2d __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_2d __attribute__((ext_vector_type(8)));
union Frag2 { f16x8_2d v; uint4 q; uint32_t d[4]; };
// Row strides chosen by the LDS banking rules (MI355X_MICROARCH.md, section LDS; scripts/dev/lds_conflicts.py does the arithmetic):
// a ds_read_b128 is served in four 16-lane groups that each hold all sixteen matrix rows, eight from one K group of the MFMA
// operand and eight from the next (+ 4 dwords).  With 68 dwords per row the sixteen 16-byte slots of a group collided pairwise
// (8 LDS cycles per read instead of 4); with 72 a row starts two slots after the previous one, the rows of one K group take the
// even slots and those of the other the odd ones.  The result tile's rows are 20 floats apart so that the four rows a
// ds_write_b32 touches per 32-lane group start 16 banks apart (17: 4 cycles per write instead of 2).  Round 5's counters had
// 43.8 M conflict cycles per launch on S6 (44 % of the LDS-active cycles): 16 per pair from the reads, 8 from the writes.
#ifndef SCORP_2D_XSTRIDE
#define SCORP_2D_XSTRIDE 72
#endif
#ifndef SCORP_2D_DSTRIDE
#define SCORP_2D_DSTRIDE 20
#endif
constexpr int k2XStride = SCORP_2D_XSTRIDE;  // dwords per row of the [16][64] value matrix (16-byte aligned rows, conflict-free row writes)
constexpr int k2DStride = SCORP_2D_DSTRIDE;  // floats per row of the 16 x 16 result tile
#ifndef SCORP_2D_TARGET_EXP
#define SCORP_2D_TARGET_EXP 12
#endif
constexpr int k2TargetExp = SCORP_2D_TARGET_EXP;   // the block's largest |upstream gradient| is scaled into [2^12, 2^13): the B operand's
                                             // gradient columns (two fp16 terms) keep 22 bits for a pixel whose gradient is down to 2^-14 of the
                                             // block's largest.  The A side does not depend on it any more: every hit's values are brought to a
                                             // fixed range by the hit's own power of two (`sg` in the kernel; until round 5 they rode on this
                                             // scale alone, [1, 2) with a factor of nine of head room for a depth-loss-dominated block at the
                                             // far plane - tests/test_gs2d_gpu.py "far_depth" - and an absolute floor of 2^-24 under them)
constexpr float k2WScale = 1024.0f;
// x -> (h1(x) | h2(x) << 16), h1 = rtz16(x), h2 = rtz16(x - h1).  h1 as an fp32 value is x with the low thirteen mantissa
// bits cleared (fp16 carries ten), so the remainder needs no conversion back and ONE v_cvt_pkrtz makes the whole dword:
// three instructions per value (it was nine per two: two packs, two conversions back, two fma, two v_perm).  Below the
// fp16 normal range (2^-14; the hit's largest value sits at 2^4 .. 2^14, see `sg`) the pair ends at the same 2^-24.
// Round 6: TWO instructions - v_cvt_pkrtz writes h1 into the low half, v_fma_mixhi_f16 forms x - h1 in fp32 (exact: the
// difference is representable) straight from that half and rounds it to fp16 into the high half of the same register.  The
// remainder is rounded to nearest where it was truncated (either way x = h1 + h2 to 2^-22 relative); a value beyond the fp16
// range (not reachable: the hit's largest is held below 1.4e4, see `sg`) now ends as inf instead of a silently wrong pair.
__device__ __forceinline__ uint32_t split_one(float x) {
  uint32_t d = pack_rtz16(x, 0.0f);
  asm("v_fma_mixhi_f16 %0, %0, -1.0, %1 op_sel_hi:[1,0,0]" : "+v"(d) : "v"(x));
  return d;
}
// What lane `o` (0..19 of either half of the wave) reads out of the result tile: out = alpha * D[row][c1] + beta * D[row][c2],
// beta one of {0, 1, ox, oy, kF * offx, kF * offy} by `bsel`; `cls`: which unscaling applies (0: 1 / (sv Sh), 1: 1 / sv, 2: 1 / (sv 2^10))
struct ReadOut { int row, c1, c2, bsel, cls; float alpha; };
__device__ __forceinline__ ReadOut read_out_of(int o) {
  ReadOut r;
  r.row = 0; r.c1 = 0; r.c2 = 0; r.bsel = 0; r.cls = 1; r.alpha = 1.0f;
  if (o < 3) { r.row = o; r.c1 = 1; r.bsel = 2; r.cls = 0; }                       // d/d pa = sum dp (x + ox)
  else if (o < 6) { r.row = o - 3; r.c1 = 2; r.bsel = 3; r.cls = 0; }              // d/d pb = sum dp (y + oy)
  else if (o < 9) { r.row = o - 6; r.cls = 0; }                                    // d/d pc
  else if (o == 9) { r.row = 3; r.cls = 0; }                                       // d/d D (zr)
  else if (o == 10) { r.row = 4; }                                                 // low-pass depth (z2)
  else if (o == 11) { r.row = 5; r.c1 = 1; r.bsel = 4; r.alpha = -kFilterInvSq; }  // kF t2 (offx - x)
  else if (o == 12) { r.row = 5; r.c1 = 2; r.bsel = 5; r.alpha = -kFilterInvSq; }
  else if (o < 16) { r.row = 7; r.c1 = 3 + (o - 13); r.c2 = 9 + (o - 13); r.bsel = 1; r.cls = 2; }    // w x dL/dn (first term + remainder)
  else if (o == 16) { r.row = 6; r.alpha = -1.0f; }                                // - sum t
  else if (o < 20) { r.row = 7; r.c1 = 6 + (o - 17); r.c2 = 12 + (o - 17); r.bsel = 1; r.cls = 2; }   // w x dL/drgb
  return r;
}

#ifndef SCORP_2D_BCHUNK
#define SCORP_2D_BCHUNK 32
#endif
constexpr int k2BChunk = SCORP_2D_BCHUNK;   // hits staged per chunk: 32 (the staging arrays are 112 bytes per hit; with 64 the wave's 11.5 KB of
                                            // LDS held the kernel at 13 waves per CU where its 124 registers allow 16: 706 -> 665 us)

// Four waves per SIMD (128 registers; every instantiation fits without scratch when asked to - left at three by the launch
// bounds the split form allocated 130).  Held to five (96 registers) it spills 26 dwords: 673 -> 740 us (same box, round 4).
#ifndef SCORP_2D_BWAVES
#define SCORP_2D_BWAVES 4
#endif
// Three forms, as for the 3-D kernel (scorp_gs2d_backward_ex, include/scorp_gs.h):
//   * SPLIT (default): the description above.
//   * kExact (SCORP_BACKWARD_EXACT_FP32): the eight values of a hit stay fp32 in the matrix, the B operand holds the basis and
//     the six upstream gradients in fp32 (nine columns), the reduction is 16 v_mfma_f32_16x16x4_f32 per pair of hits.  No
//     fp16 terms, so none of the three power-of-two scales either (wave, hit, 1 / p.z): every operand is the fp32 number the
//     reference's arithmetic would carry.  The fp32 MFMA runs at the vector rate (34 cycles each): this
//     form pays 8 of them per hit where the split form pays 2 fp16 ones, and saves the split's ~40 instructions.
//   * kDet (SCORP_BACKWARD_DETERMINISTIC): the twenty sums of a (block, hit) leave as one plain row
//     partial[4 * pair + block] (pair = the (surfel, tile) pair's ordinal in surfel-major order, pair_rank in common.hpp)
//     with a flag byte; reduce_pair_rows_kernel (binning.hip) adds a surfel's rows in a fixed order.  No float atomics.
template <bool kHasMap, bool kExact = false, bool kDet = false>
__global__ void __launch_bounds__(64, SCORP_2D_BWAVES)
blend2d_backward_wave_kernel(const uint32_t *__restrict__ tile_start, const uint32_t *__restrict__ point_list,
                             const Surfel *__restrict__ rec, uint32_t capacity, int W, int H, int tiles_x, int tiles,
                             const float *__restrict__ bg, const float *__restrict__ final_T,
                             const uint32_t *__restrict__ n_contrib, const float *__restrict__ dL_dcolor,
                             const float *__restrict__ dL_dallmap, float *__restrict__ acc,
                             const uint32_t *__restrict__ hits, float *__restrict__ partial, uint8_t *__restrict__ row_flags,
                             const uint32_t *__restrict__ pair_base, const BinRec *__restrict__ bin,
                             const uint64_t *__restrict__ tile_mask) {
  __shared__ float4 q0[k2BChunk], q1[k2BChunk], q2[k2BChunk], q3[k2BChunk], q4[k2BChunk];
  __shared__ float2 q5[k2BChunk];                        // q0..q3: SurfelLin, q4: (normal, r), q5: (g, b)
  __shared__ uint32_t q_id[k2BChunk], q_pos[k2BChunk];
  __shared__ float q6[k2BChunk];                         // Sh: the hit's power-of-two scale for the 1 / p.z values (0: taken at replay)
  // what the read-out lanes multiply with, one row of eight floats per hit, formed once by the staging lane:
  // [0, 1, ox, oy, kF (cx - bxc), kF (cy - byc), 1 / Sh, 1] - a lane picks its two entries by index (it was five selects)
  __shared__ __attribute__((aligned(16))) float q7[k2BChunk * 8];
  // [row = hit of the pair x kind][pixel] matrix of (h1 | h2 << 16) dwords; the 16 x 16 result tile reuses its first rows
  __shared__ __attribute__((aligned(16))) uint32_t xm2[16 * k2XStride];
  float *dbuf = reinterpret_cast<float *>(xm2);
  static_assert(16 * k2DStride <= 16 * k2XStride && 64 * 6 <= 16 * k2XStride, "the result tile and the prologue scratch fit the matrix");
  const int lane = threadIdx.x;
  BlockWave blk;
  if (!block_wave(tiles, tiles_x, blk)) return;
  const int tile = blk.tile, quad = blk.quad, bx = blk.bx, by = blk.by;
  const int px = bx + (lane & 7), py = by + (lane >> 3);
  const bool inside = px < W && py < H;
  const float pxf = (float)px, pyf = (float)py;
  const float bxc = (float)bx + 3.5f, byc = (float)by + 3.5f;                    // the linear form's expansion point (surfel_lin)
  const float qxb = (float)(lane & 7) - 3.5f, qyb = (float)(lane >> 3) - 3.5f;   // this pixel about it
  const TileRange tr = tile_range(tile_start, tile, capacity);
  if (tr.end == tr.beg) return;
  const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
  // all of the pixel's loads are issued together; pixels nothing was blended into drop their upstream gradient
  // afterwards by a select (it may be NaN)
  float T_final = 0, final_D = 0, final_D2 = 0, dpix0 = 0, dpix1 = 0, dpix2 = 0, ddep = 0, dacc = 0, dn0 = 0, dn1 = 0, dn2 = 0,
        dmed = 0, dreg = 0;
  uint32_t last = 0, med_c = 0;
  if (inside) {
    T_final = final_T[pix];
    last = n_contrib[pix];
    dpix0 = dL_dcolor[pix]; dpix1 = dL_dcolor[HW + pix]; dpix2 = dL_dcolor[2 * HW + pix];
    if (kHasMap) {
      final_D = final_T[HW + pix]; final_D2 = final_T[2 * HW + pix];
      med_c = n_contrib[HW + pix];
      ddep = dL_dallmap[pix]; dacc = dL_dallmap[HW + pix];
      dn0 = dL_dallmap[2 * HW + pix]; dn1 = dL_dallmap[3 * HW + pix]; dn2 = dL_dallmap[4 * HW + pix];
      dmed = dL_dallmap[5 * HW + pix]; dreg = dL_dallmap[6 * HW + pix];
    }
  }
  if (last == 0) { final_D = final_D2 = dpix0 = dpix1 = dpix2 = ddep = dacc = dn0 = dn1 = dn2 = dmed = dreg = 0.0f; med_c = 0; }
  const float final_A = 1.0f - T_final;
  const float fn = kFarZ / (kFarZ - kNearZ);
  uint32_t todo = last;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) todo = max(todo, (uint32_t)__shfl_xor((int)todo, off, 64));
  todo = (uint32_t)__builtin_amdgcn_readfirstlane((int)todo);   // wave-uniform: keeps the chunk loop's counters in SGPRs
  // one power-of-two scale per wave from the block's largest upstream gradient (exact; everything below is linear in them)
  float sv = 1.0f, inv_sv = 1.0f;
  if constexpr (!kExact) {
    float amax = fmaxf(fmaxf(fabsf(dpix0), fabsf(dpix1)), fabsf(dpix2));
    if (kHasMap) amax = fmaxf(fmaxf(fmaxf(amax, fabsf(ddep)), fmaxf(fabsf(dacc), fabsf(dmed))),
                              fmaxf(fmaxf(fabsf(dn0), fabsf(dn1)), fmaxf(fabsf(dn2), fabsf(dreg))));
    const int eb = (int)((wave_max_u32(__float_as_uint(amax)) >> 23) & 0xFFu);   // biased exponent; 0: zero / denormal
    const int sb = eb == 0 ? 127 : min(max(254 + k2TargetExp - eb, 1), 253);
    sv = __uint_as_float((uint32_t)sb << 23);
    inv_sv = __uint_as_float((uint32_t)(254 - sb) << 23);
  }
  dpix0 *= sv; dpix1 *= sv; dpix2 *= sv; ddep *= sv; dacc *= sv; dn0 *= sv; dn1 *= sv; dn2 *= sv; dmed *= sv; dreg *= sv;
  // (of the SCALED gradients, like everything below); per-pixel constants of the recurrence formed once: T_final bg . dL/dc,
  // and the distortion term's final_A, final_D, final_D2 with the map's upstream gradient folded in
  const float tf_bg = T_final * (bg[0] * dpix0 + bg[1] * dpix1 + bg[2] * dpix2);
  const float far_ = final_A * dreg, fdr_ = final_D * dreg, fd2r_ = final_D2 * dreg;
  // B operand.  A lane supplies ONE column bn of the basis for the pixels 16 m + 4 bk + j (MFMA m, j = 0..3), each value twice
  // (once per fp16 term of the A side).  The six gradient columns come from the other lanes through LDS (the matrix is idle).
  Frag2 bh[kExact ? 1 : 4];
  float bb[kExact ? 16 : 1];   // exact form: fp32 MFMA 4 m + j covers the pixels 16 m + 4 bk + j (one per K slot bk)
  {
    float *xs = reinterpret_cast<float *>(xm2);
    xs[lane * 6 + 0] = dn0; xs[lane * 6 + 1] = dn1; xs[lane * 6 + 2] = dn2;
    xs[lane * 6 + 3] = dpix0; xs[lane * 6 + 4] = dpix1; xs[lane * 6 + 5] = dpix2;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int bn = lane & 15, bk = lane >> 4;
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int q = 16 * m + 4 * bk + j;
        float b = 0.0f;
        b = bn == 0 ? 1.0f : b;
        b = bn == 1 ? (float)(q & 7) - 3.5f : b;
        b = bn == 2 ? (float)(q >> 3) - 3.5f : b;
        if constexpr (kExact) {
          if (bn >= 3 && bn <= 8) b = xs[q * 6 + (bn - 3)];   // columns 3..8: the six upstream gradients, whole; 9..15: zero
          bb[4 * m + j] = b;
        } else {
          if (bn >= 3 && bn <= 14) {
            const float g = xs[q * 6 + (bn - 3) % 6];
            const float g1 = half_lo(pack_rtz16(g, 0.0f));
            b = bn <= 8 ? g1 : g - g1;                       // columns 3..8: first fp16 term, 9..14: the remainder
          }
          const uint32_t hb = pack_rtz16(b, 0.0f) & 0xFFFFu;
          bh[m].d[j] = hb | (hb << 16);
        }
      }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const ReadOut ro = read_out_of(lane & 31);
  const int ro_beta = ro.bsel, ro_us = kExact ? 7 : (ro.cls == 0 ? 6 : 7);   // this lane's entries of a hit's q7 row
  constexpr float kWCarry = kExact ? 1.0f : k2WScale;   // the blend weight travels as w * 2^10 in the split form only
  const float ro_unscale = ro.cls == 2 ? inv_sv * (1.0f / kWCarry) : inv_sv;
  const int abase = (lane & 15) * k2XStride + 4 * (lane >> 4);
  // Two hits per pass over the matrix pipe: `pend` halves of the matrix are filled (slots pend_s[0], pend_s[1] of the chunk)
  int pend = 0, pend_s0 = 0, pend_s1 = 0;
  float pend_iw0 = 1.0f, pend_iw1 = 1.0f;   // 1 / (the hit's block-floating-point scale, see `sg` below)
  uint64_t pend_live = 0;                   // exact form: the pixels either hit of the pair is live on (wave-uniform)
  auto flush_pair = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f32x4_2d d = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (kExact) {
      float4 av[4];
#pragma unroll
      for (int m = 0; m < 4; m++) av[m] = *reinterpret_cast<const float4 *>(&xm2[abase + 16 * m]);
      // MFMAs 4 m .. 4 m + 3 cover the pixels 16 m .. 16 m + 15 (two rows of the block).  A surfel's footprint is a few pixels
      // across: where neither hit of the pair is live on those two rows every A value is an exact zero and the four fp32
      // MFMAs (34 cycles each at the vector rate) are skipped - a wave-uniform branch on the pair's live-pixel mask.
#pragma unroll
      for (int m = 0; m < 4; m++) {
        if (((pend_live >> (16 * m)) & 0xFFFFull) != 0) {
          d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].x, bb[4 * m], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].y, bb[4 * m + 1], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].z, bb[4 * m + 2], d, 0, 0, 0);
          d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m].w, bb[4 * m + 3], d, 0, 0, 0);
        }
      }
    } else {
      Frag2 af[4];
#pragma unroll
      for (int m = 0; m < 4; m++) af[m].q = *reinterpret_cast<const uint4 *>(&xm2[abase + 16 * m]);
#pragma unroll
      for (int m = 0; m < 4; m++) d = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[m].v, bh[m].v, d, 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();   // every lane has its A operands: the result tile may overwrite the matrix
#pragma unroll
    for (int i = 0; i < 4; i++) dbuf[(4 * (lane >> 4) + i) * k2DStride + (lane & 15)] = d[i];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int hh = lane >> 5;
    if ((lane & 31) < kAcc2Stride && hh < pend) {   // lanes 0..19: the first hit of the pair, 32..51: the second
      const int sl = hh ? pend_s1 : pend_s0;
      const float beta = q7[sl * 8 + ro_beta];
      const float *row = dbuf + (ro.row + 8 * hh) * k2DStride;
      float v = ro.alpha * row[ro.c1] + beta * row[ro.c2];
      if constexpr (!kExact) v = v * (ro_unscale * q7[sl * 8 + ro_us]) * (hh ? pend_iw1 : pend_iw0);
      if constexpr (kDet) {   // (q_id holds the pair's ordinal; one beyond the reservation: an overflowed view, discarded anyway)
        const uint32_t pair = q_id[sl];
        if (pair < capacity) {
          const size_t r = (size_t)pair * 4u + (uint32_t)quad;
          partial[r * kAcc2Stride + (lane & 31)] = v;   // whole rows, zeros included: nothing was cleared beforehand
          if ((lane & 31) == 0) row_flags[r] = 1;
        }
      } else {
        atomicAdd(acc + (size_t)q_id[sl] * kAcc2Stride + (lane & 31), v);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the next hits' rows overwrite the result tile
    pend = 0;
  };
  float T = T_final, R = 0.0f, s_last = 0.0f, last_alpha = 0.0f, last_dL_dT = 0.0f;
  // Block floating point per hit.  The fp16 pair x = h1 + h2 has an ABSOLUTE floor (2^-24, the last denormal): against the
  // block's largest upstream gradient scaled into [1, 2) a hit at the rim of a faint surfel (alpha ~ 0.004, T ~ 0.3: values
  // ~ 1e-3) was left with 14 bits, a hit deep in a list with fewer - invisible in a tensor's max norm, percent-level in
  // the row of a surfel that only such pixels see (2-D fuzz, seeds 63 / 64: tests/test_gs2d_gpu.py).  All eight values
  // are linear in the three per-pixel roots (t, dL/dz, w); the largest |root| over the hit's pixels (one wave maximum)
  // gives the power of two `sg` that brings it into [2^4, 2^5) - wave-uniform, exact, undone at the read-out - so the
  // pair keeps its 22 bits down to 2^-17 of the hit's largest value, whatever T, alpha or the depth scale are.
  // Range: |dp| <= 12 |t| (|1 / p.z| Sh <= 4, |s| <= 3), |dp2| <= 36 |t| + 400 |dL/dz| (depth <= kFarZ): 1.4e4 at most;
  // w * 2^10 <= 2^15.
  // gathers software-pipelined two chunks deep over the block's hit list (left by the forward), back to front: lane l of
  // the chunk that starts dn hits from the end takes the hit at 0-based position todo - 1 - dn - l
  const uint32_t *my_hits = block_hit_list(hits, quad, capacity, tr.beg);
  auto fetch_idx = [&](uint32_t dn, bool &hit_, uint32_t &id_) {
    hit_ = lane < k2BChunk && dn + lane < todo;
    id_ = hit_ ? my_hits[todo - 1 - dn - lane] : 0u;
  };
  auto fetch_rec = [&](bool hit_, uint32_t id_, float4 &a0_, float4 &a1_, float4 &a2_, float4 &a3_, float4 &a4_) {
    if (hit_) {
      const float4 *src = reinterpret_cast<const float4 *>(rec + id_);
      a0_ = src[0]; a1_ = src[1]; a2_ = src[2]; a3_ = src[3]; a4_ = src[4];
    }
  };
  bool hit, hit1;
  uint32_t id, id1;
  float4 r0, r1, r2, r3, r4;
  fetch_idx(0, hit, id);
  fetch_rec(hit, id, r0, r1, r2, r3, r4);
  fetch_idx(k2BChunk, hit1, id1);
  for (uint32_t done_n = 0; done_n < todo; done_n += k2BChunk) {
    const uint32_t top = todo - 1 - done_n;
    float4 nx0, nx1, nx2, nx3, nx4;   // next chunk's records
    fetch_rec(hit1, id1, nx0, nx1, nx2, nx3, nx4);
    bool hit2;
    uint32_t id2;
    fetch_idx(done_n + 2 * k2BChunk, hit2, id2);
    __builtin_amdgcn_wave_barrier();   // every lane is past the previous chunk's reads of the ring
    if (hit) {   // (the chunk's hits are lanes 0 .. cnt-1: a hit list has no gaps)
      const int qi = lane;
      const SurfelLin L = surfel_lin(r0, r1, r2, bxc, byc);
      q0[qi] = L.e0; q1[qi] = L.e1; q2[qi] = L.e2; q3[qi] = L.e3; q4[qi] = r3;
      // (ox, oy) = block centre - the surfel's accumulation point (its centre clamped into the image)
      q5[qi] = make_float2(r4.x, r4.y);
      float sh_stage = 1.0f, ish_stage = 1.0f;
      if constexpr (kDet) {
        // the (surfel, tile) pair's ordinal, surfel-major (pair_rank)
        const uint4 raw = reinterpret_cast<const uint4 *>(bin)[id];
        const BinRec br = *reinterpret_cast<const BinRec *>(&raw);
        const uint64_t mk = tile_mask[id];
        q_id[qi] = pair_base[id] + pair_rank(br, mk, blk.tx, blk.ty);
      } else {
        q_id[qi] = id;
      }
      q_pos[qi] = top - (uint32_t)lane + 1u;
      // The power of two below |p.z| at the block centre (L.e2.x): 1 / p.z times it stays within [1/3, 4] over the block as
      // long as p.z = e2.x + e0.z qx + e1.y qy (|qx|, |qy| <= 3.5) stays within half of its centre value.  Where it does not - a
      // large surfel whose horizon passes near the block - the centre says nothing about the pixels that count, and the
      // scale is taken from the hit's largest |1 / p.z| over its valid pixels when the hit is replayed (Sh = 0 asks for it).
#ifndef SCORP_2D_STEADY_FRAC
#define SCORP_2D_STEADY_FRAC 0.5f
#endif
      if constexpr (!kExact) {
        const float pzc = fabsf(L.e2.x);
        const bool steady = 3.5f * (fabsf(L.e0.z) + fabsf(L.e1.y)) <= SCORP_2D_STEADY_FRAC * pzc;
        const uint32_t eb = min(max(__float_as_uint(pzc) & 0x7F800000u, 0x10000000u), 0x6F000000u);
        sh_stage = steady ? __uint_as_float(eb) : 0.0f;
        ish_stage = __uint_as_float(0x7F000000u - eb);
        q6[qi] = sh_stage;
      }
      float4 *tb = reinterpret_cast<float4 *>(q7 + 8 * qi);
      tb[0] = make_float4(0.0f, 1.0f, bxc - fminf(fmaxf(r2.y, 0.0f), (float)(W - 1)), byc - fminf(fmaxf(r2.z, 0.0f), (float)(H - 1)));
      tb[1] = make_float4(kFilterInvSq * (L.e2.z - bxc), kFilterInvSq * (L.e2.w - byc), ish_stage, 1.0f);
    }
    const int cnt = (int)min(todo - done_n, (uint32_t)k2BChunk);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int s_ = 0; s_ < cnt; s_++) {
      int s = s_;
      asm volatile("" : "+v"(s));   // one VGPR slot index: the ds_reads below share it instead of re-moving SGPR bases
      const uint32_t pos1 = q_pos[s];
      const float4 a0 = q0[s], a1 = q1[s], a2 = q2[s], a3 = q3[s];
      Eval2 h;
      const bool valid = eval_surfel(a0, a1, a2, a3, qxb, qyb, pxf, pyf, h) & (pos1 <= last);
      const uint64_t live = __ballot(valid);
      if (live == 0) continue;
      // The per-pixel recurrence runs under `valid`; it leaves three scalars (blend weight w, t = dL/dG * (-G), dL/dz)
      // that are zero on the other lanes, and the twenty sums are formed from them outside the branch with the
      // geometry zeroed where it is not used (pz ~ 0 makes s, rz, depth non-finite there), so no lane ever needs
      // its twenty accumulators cleared first.
      float w = 0.0f, t = 0.0f, dL_dz = 0.0f;
      const float4 nr = q4[s];
      const float2 gb = q5[s];
      if (valid) {
        const float rinv = __builtin_amdgcn_rcpf(1.0f - h.alpha);
        T *= rinv;
        w = h.alpha * T;
        // the "blended behind" recurrences (colour, depth, alpha, normal) only ever appear dotted with this pixel's
        // upstream gradient, so one scalar recurrence carries them all (see gs3d_backward.hip)
        R = last_alpha * (s_last - R) + R;
        float sc = nr.w * dpix0 + gb.x * dpix1 + gb.y * dpix2;
        if (kHasMap) sc += h.depth * ddep + dacc + nr.x * dn0 + nr.y * dn1 + nr.z * dn2;
        float dL_dal = sc - R;
        s_last = sc;
        if (kHasMap) {
          // distortion: dL/dweight = dreg (D2 + m^2 A - 2 m D) = fd2r + m (u - fdr), u = m far - fdr (also the depth term's factor)
          const float rd = h.rdepth;
          const float m_d = __builtin_fmaf(-fn * kNearZ, rd, fn);
          const float dmd_dd = ((kFarZ * kNearZ / (kFarZ - kNearZ)) * rd) * rd;
          const float u = __builtin_fmaf(m_d, far_, -fdr_);
          const float dL_dweight = __builtin_fmaf(m_d, u - fdr_, fd2r_);
          dL_dz = (pos1 == med_c) ? dmed : 0.0f;
          dL_dal += dL_dweight - last_dL_dT;
          last_dL_dT = dL_dweight * h.alpha + (1.0f - h.alpha) * last_dL_dT;
          dL_dz = __builtin_fmaf(w + w, u * dmd_dd, dL_dz);
          dL_dz = __builtin_fmaf(w, ddep, dL_dz);
        }
        dL_dal *= T;
        last_alpha = h.alpha;
        dL_dal = __builtin_fmaf(-tf_bg, rinv, dL_dal);
        t = -h.Go * dL_dal;          // dL/dG * (-G), G = Go / opacity
      }
      float inv_sg = 1.0f;
      if constexpr (!kExact) {   // the hit's power-of-two scale (see above); a hit whose roots are all zero or denormal keeps 1
        const uint32_t eb = wave_max_u32(__float_as_uint(fmaxf(fmaxf(fabsf(t), fabsf(dL_dz)), w))) >> 23;
        const uint32_t sb = eb == 0u ? 127u : min(258u - eb, 250u);   // 2^(4 - (eb - 127)), biased
        const float sg = __uint_as_float(sb << 23);
        inv_sg = __uint_as_float((254u - sb) << 23);
        t *= sg; dL_dz *= sg; w *= sg;
      }
      // The eight per-pixel values of this hit (zero on the lanes it does not touch), as two fp16 terms each, into the
      // matrix half `pend`; the products with the bases and the sums over the block's pixels are the matrix cores' work.
      {
        const bool u3 = valid & h.use3d;
        const float s0 = u3 ? h.s0 : 0.0f, s1 = u3 ? h.s1 : 0.0f, dep = u3 ? h.depth : 0.0f;
        float Sh = 1.0f;
        if constexpr (!kExact) Sh = q6[s];                                  // (wave-uniform: one LDS broadcast)
        if (!kExact && Sh == 0.0f) {   // no steady scale for this hit (see the staging): 2^-e of its largest |1 / p.z| over the valid 3-D pixels
          const uint32_t em = min(max(wave_max_u32(u3 ? (__float_as_uint(h.rz) & 0x7F800000u) : 0u), 0x10000000u), 0x6F000000u);
          Sh = __uint_as_float(0x7F000000u - em);
          if (lane == 0) q7[8 * s_ + 6] = __uint_as_float(em);                // the read-out unscales with it
        }
        const float rzs = u3 ? h.rz * Sh : 0.0f;                            // 1 / p.z times the hit's power-of-two scale
        const float t2 = h.use3d ? 0.0f : t, z2 = h.use3d ? 0.0f : dL_dz;   // low-pass branch (t, dL_dz are 0 if !valid)
        const float tr = t * rzs;
        const float dp0 = tr * s0, dp1 = tr * s1;
        const float zr = dL_dz * rzs;                                       // depth = D / pz
        const float dp2 = -(dp0 * s0 + dp1 * s1) - zr * dep;
        uint32_t *rowp = xm2 + (8 * pend) * k2XStride + lane;
        auto term = [](float x) { return kExact ? __float_as_uint(x) : split_one(x); };
        rowp[0] = term(dp0); rowp[k2XStride] = term(dp1);
        rowp[2 * k2XStride] = term(dp2); rowp[3 * k2XStride] = term(zr);
        rowp[4 * k2XStride] = term(z2); rowp[5 * k2XStride] = term(t2);
        rowp[6 * k2XStride] = term(t); rowp[7 * k2XStride] = term(w * kWCarry);
      }
      if (pend == 0) { pend_s0 = s_; pend_iw0 = inv_sg; pend_live = live; } else { pend_s1 = s_; pend_iw1 = inv_sg; pend_live |= live; }
      pend++;
      if (pend == 2) flush_pair();
    }
    if (pend) flush_pair();   // (before the next chunk's staging overwrites the slots the read-out looks at)
    hit = hit1; id = id1; r0 = nx0; r1 = nx1; r2 = nx2; r3 = nx3; r4 = nx4;
    hit1 = hit2; id1 = id2;
  }
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_gs2d_backward_scratch_bytes(int32_t N) { return backward_scratch_bytes(N, 0, 0u, kAcc2Stride); }
extern "C" size_t scorp_gs2d_backward_scratch_bytes_ex(int32_t N, int32_t W, int32_t H, uint64_t capacity, uint32_t flags) {
  (void)W; (void)H;
  return backward_scratch_bytes(N, capacity, flags, kAcc2Stride);
}

extern "C" int scorp_gs2d_backward(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                                   const float *dL_dcolor, const float *dL_dallmap, const ScorpGs3dGrads *grads,
                                   void *scratch, size_t scratch_bytes, scorp_stream_t stream_) {
  return scorp_gs2d_backward_ex(in, state, pairs, capacity, dL_dcolor, dL_dallmap, grads, scratch, scratch_bytes, 0u, stream_);
}

// (2DGS ignores SCORP_BACKWARD_SCRATCH_ZEROED: include/scorp_gs.h)
extern "C" int scorp_gs2d_backward_ex(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                                      const float *dL_dcolor, const float *dL_dallmap, const ScorpGs3dGrads *grads,
                                      void *scratch, size_t scratch_bytes, uint32_t flags, scorp_stream_t stream_) {
  return backward2d_impl(in, state, pairs, capacity, dL_dcolor, dL_dallmap, grads, scratch, scratch_bytes,
                         flags & ~SCORP_BACKWARD_SCRATCH_ZEROED, stream_, nullptr);
}

// `adam` (scorp_gs2d_train_view): the per-surfel kernel applies the optimizer step and the view's statistics itself
int scorp::backward2d_impl(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                           const float *dL_dcolor, const float *dL_dallmap, const ScorpGs3dGrads *grads, void *scratch,
                           size_t scratch_bytes, uint32_t flags, scorp_stream_t stream_, const AdamEpi *adam,
                           float lambda_isotropic) {
  hipStream_t stream = (hipStream_t)stream_;
  const char *base = (const char *)state, *pb = (const char *)pairs;
  auto blend = [&](const StateLayout &L, const PairLayout &P, float *acc, float *partial, uint8_t *row_flags, uint32_t *pair_base) {
    const bool det = partial != nullptr, exact = (flags & SCORP_BACKWARD_EXACT_FP32) != 0, map = dL_dallmap != nullptr;
    auto wk = det ? (exact ? (map ? blend2d_backward_wave_kernel<true, true, true> : blend2d_backward_wave_kernel<false, true, true>)
                           : (map ? blend2d_backward_wave_kernel<true, false, true> : blend2d_backward_wave_kernel<false, false, true>))
                  : (exact ? (map ? blend2d_backward_wave_kernel<true, true, false> : blend2d_backward_wave_kernel<false, true, false>)
                           : (map ? blend2d_backward_wave_kernel<true, false, false> : blend2d_backward_wave_kernel<false, false, false>));
    wk<<<block_wave_grid(L.tiles), 64, 0, stream>>>(
        (const uint32_t *)(base + L.tile_start), (const uint32_t *)(pb + P.list), (const Surfel *)(base + L.rec),
        (uint32_t)capacity, in->image_width, in->image_height, L.tiles_x, L.tiles, in->bg, (const float *)(base + L.final_T),
        (const uint32_t *)(base + L.n_contrib), dL_dcolor, dL_dallmap, acc, (const uint32_t *)(pb + P.hits), partial, row_flags,
        pair_base, (const BinRec *)(base + L.bin), (const uint64_t *)(base + L.tile_mask));
  };
  auto per_gaussian = [&](const StateLayout &L, const float *acc) {
    launch_preprocess2d_backward(in, L, (const Surfel *)(base + L.rec), (const BinRec *)(base + L.bin), acc, grads, stream, adam,
                                 lambda_isotropic);
  };
  return backward_pass(kGs2d, in, state, pairs, capacity, dL_dcolor, grads, scratch, scratch_bytes, flags, stream, blend,
                       per_gaussian);
}
