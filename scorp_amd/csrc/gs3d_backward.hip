// gs3d_backward.hip — 3DGS backward for gfx950: per-tile back-to-front replay -> per-Gaussian chain rule.
//
// Replaces the backward half of `diff_gaussian_rasterization` (reached from `loss.backward()`,
// train_3dgs.py:152; colour-only at post_refine_gs.py:53-56; w.r.t. colors_precomp at utils/mask.py:47-70).
// Arithmetic follows oracle/gs3d_oracle.c::gs3d_oracle_backward.  The forward state and the pair buffer are
// only read, so the backward can be replayed on one forward.

#include <type_traits>

#include "common.hpp"
#include "exp_mfma.hpp"

namespace scorp {
namespace {

// ---------------------------------------------------------------------------------------------------------
// The blend backward: a back-to-front replay of each pixel's blend with the pixel->splat reduction done on the
// matrix cores.
//
// For one splat the ten sums over pixels factor as  sum_p v_p * {1, x_p, y_p, x_p^2, x_p y_p, y_p^2}  (geometry:
// v_p = G * opacity * dL/dalpha, pixel coordinates relative to the block centre) and  sum_p w_p * {dL/dr, dL/dg, dL/db,
// dL/ddepth}_p  (w_p = alpha * T).  With a wave's 64 pixels as the K dimension that is
// D[16 splats][16 columns] = [V | W] * [basis_v ; basis_w].
//
// Per wave and 16-splat group:
//   1a (straight-line, no dependence between splats): alpha and G*opacity of the 16 splats at this lane's pixel;
//   1b (the sequential part): T, the blended-behind recurrence and dL/dalpha.  A splat that does not contribute to
//      this pixel is carried through as alpha = 0, which leaves every recurrence bit-for-bit unchanged, so the
//      group is branch-free.  The five "accumulated colour/depth/alpha behind" recurrences of the textbook form
//      collapse into ONE, because only their dot product with this pixel's upstream gradient is ever used:
//      s = c.dL/dcolor + z*dL/ddepth + dL/dalpha,  R <- last_alpha * s_last + (1 - last_alpha) * R,
//      dL/dalpha_i = (s - R) * T - T_final / (1 - alpha) * (bg . dL/dcolor);
//   lane (= pixel) writes v, w into two wave-private LDS matrices [slot][pixel] (row stride 68 dwords: conflict-free
//   row writes, 16-byte-aligned rows for the transposed A-operand reads);
//   the matrix result holds block-frame moments, which stay in the splats' staging entries until the wave's chunk of 64
//   hits is done; then ONE pass (lane = splat) turns them into the ten screen-space gradients, and they are flushed with
//   float atomics shaped as whole 40-byte row segments (lanes = consecutive floats).
//
// Two forms of the reduction (template parameter kExact, entry point scorp_gs3d_backward_ex):
//   * SPLIT (default): v and w leave the lane as TWO fp16 terms each - h1 = rtz16(x), h2 = rtz16(x - h1), 22 bits
//     together (fp32 carries 24) - packed (v | w) into one dword per term, so a slot costs one ds_write2_b32.  With
//     K = (pixel, v-or-w) the whole reduction is 8 v_mfma_f32_16x16x32_f16 per group (two passes, one per term, over
//     ONE B operand): columns 0..5 hold the position basis (half-integer block coordinates and their products, exact
//     in fp16) against the v slots, columns 6..9 / 10..13 the high / low fp16 term of the upstream gradients against
//     the w slots.  The products are exact and accumulate in fp32.  Range: the pixel's upstream gradients are
//     pre-scaled by a power of two chosen per wave from the block's largest |dL/dpixel| (so v sits around 2^7 ... and
//     the conversion saturates, RTZ, instead of overflowing), w by 2^10; the sums are unscaled by exact powers of two.
//   * EXACT (kExact): v and w stay fp32 and go through v_mfma_f32_4x4x1_16b_f32 (16 independent 4x4 blocks, K = 1, each
//     with its own A and B; 8 cycles per instruction, scripts/mb_mfma_4x4.hip).  Per half-group of 8 hits, block
//     (hit quad qb, pixel row rb) and instruction k = pixel column: A = v (w) of hit 4 qb + i at pixel (k, rb), B = column
//     j at that pixel - {1, x, x^2, y} for v, the four upstream gradients for w - so 8 + 8 instructions per half, 32 per
//     group (256 matrix cycles; the 16x16x4 form took 32 x 32 = 1 024, two thirds of its MACs unused).  The rows' partial
//     sums are added across lanes (two permlane swaps, each pairing two registers, and one DPP add), with the y-weighted
//     sums (y x v, y^2 v) formed on the way.  Products are exact fp32, accumulation fp32 (only the order changes).  The
//     parity tests compare the two forms with each other and each with the oracle.
// ---------------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
#ifndef SCORP_BWD_XSTRIDE
#define SCORP_BWD_XSTRIDE 68
#endif
constexpr int kXStride = SCORP_BWD_XSTRIDE;  // dwords per slot row of the wave-private matrices: rows stay 16-byte
                                             // aligned for the A-operand's ds_read_b128; row writes are conflict-free
constexpr int kGroup = 16;                   // splats per MFMA group
#ifndef SCORP_BWD_DSTRIDE
#define SCORP_BWD_DSTRIDE 20
#endif
constexpr int kDStride = SCORP_BWD_DSTRIDE;   // floats per slot row of the 16 x 14 result tile: 20 (80 bytes, 16-byte aligned rows) keeps the
                                             // sixteen moment lanes' 16-byte row reads on distinct banks (stride 16: lanes 0, 4, 8, 12 collide)
constexpr float kLog2e = 1.4426950408889634f;
constexpr int kVTargetExp = 7;               // split form: the block's largest |dL/dpixel| is scaled into [2^7, 2^8)
constexpr int kVTargetExpDA = 4;             // ... [2^4, 2^5) when depth / alpha gradients (depth values!) take part
constexpr float kWScale = 1024.0f;           // split form: blend weights (<= 1) are carried as w * 2^10

// ---------------------------------------------------------------------------------------------------------
// B1w: the replay with ONE WAVE PER 8x8 PIXEL BLOCK as the unit of work (64-thread workgroups, no workgroup
// barriers, no waiting for the slowest wave of a tile).  A wave walks its block's HIT LIST (left by the forward: the
// splats that passed the exact ellipse-vs-block test, compacted, in blend order) back to front 64 hits at a time: each
// lane gathers one record (list entries are fetched two chunks ahead, records one) into a 64-slot staging buffer in the
// wave's own LDS, and the chunk's four groups of 16 go through the 1a / 1b / MFMA pipeline described above.  A hit's
// position in the list is arithmetic (no per-slot position array): slot i of a group whose first slot has 1-based
// position `top` belongs to the pixel's blend iff top - i <= last contributor of the pixel.  A group ends with its hits'
// block-frame moments in the hits' own staging entries (the exact form's row sums land there directly, the split form adds
// its two terms per group).  The tail runs once per chunk: every lane converts one hit's moments to the ten gradients
// (the same instructions as a per-group tail on sixteen lanes, issued a quarter as often) and leaves them as a row of the
// idle matrix; the chunk's 64 rows are added to the per-Gaussian accumulators with up to sixteen wave-wide float atomics
// (four rows each, zero terms skipped) while the next chunk is being staged, and after the loop for the last chunk.
// Blocks are numbered so that the four waves of a tile land on the same XCD (same L2).
// ---------------------------------------------------------------------------------------------------------
constexpr int kChunk = 64;
constexpr int kRStride = 12;                  // floats per row of a chunk's 64 x 10 results: 16-byte aligned rows, and the four rows
                                             // a flush instruction reads (ten floats each, 12 apart) sit on distinct banks

#ifndef SCORP_BWD_WAVES
#define SCORP_BWD_WAVES 4
#endif
// kHasDA false: no upstream gradient on the depth / alpha images (the photometric-loss-only step).
// kColorOnly: only dL/dcolour is wanted (post_refine_gs.py:53-56 freezes xyz / scale / rotation / opacity and trains SH0):
// no dL/dalpha, no "blended behind" recurrence, no v; the matrix rows carry w alone, three sums per splat leave.
// fp16 bits of the V columns of the B operand: kBasisV[bn][q] = column bn (1, x, y, x^2, xy, y^2 in the block frame, half-
// integer coordinates: exact) at pixel q of the 8x8 block.  A lane's sixteen values are consecutive (q = 16 bk .. + 15).
struct BasisTable { uint16_t v[6][64]; };
constexpr uint16_t f16_bits_small(float x) {   // exact for the multiples of 0.25 below 16 that occur here
  if (x == 0.0f) return 0;
  const uint16_t sign = x < 0.0f ? 0x8000u : 0u;
  float a = x < 0.0f ? -x : x;
  int e = 15;
  while (a >= 2.0f) { a *= 0.5f; e++; }
  while (a < 1.0f) { a *= 2.0f; e--; }
  return (uint16_t)(sign | (e << 10) | (uint16_t)((a - 1.0f) * 1024.0f));
}
constexpr BasisTable make_basis_table() {
  BasisTable t{};
  for (int q = 0; q < 64; q++) {
    const float xl = (float)(q & 7) - 3.5f, yl = (float)(q >> 3) - 3.5f;
    const float col[6] = {1.0f, xl, yl, xl * xl, xl * yl, yl * yl};
    for (int c = 0; c < 6; c++) t.v[c][q] = f16_bits_small(col[c]);
  }
  return t;
}
__device__ const BasisTable kBasisV = make_basis_table();

// kDet: SCORP_BACKWARD_DETERMINISTIC - the sums leave as plain rows partial[quad][hit-list position] instead of float atomics
template <bool kHasDA, bool kExact, bool kColorOnly = false, bool kDet = false>
__global__ void __launch_bounds__(64, SCORP_BWD_WAVES)
blend_backward_wave_kernel(const uint32_t *__restrict__ tile_start, const uint32_t *__restrict__ hits,
                           const SplatRec *__restrict__ rec, uint32_t capacity, int W, int H, int tiles_x, int tiles,
                           const float *__restrict__ bg, const float *__restrict__ final_T,
                           const uint32_t *__restrict__ n_contrib, const float *__restrict__ dL_dcolor,
                           const float *__restrict__ dL_ddepth, const float *__restrict__ dL_dalpha,
                           float *__restrict__ acc, float *__restrict__ partial, uint8_t *__restrict__ row_flags,
                           const uint32_t *__restrict__ pair_base, const BinRec *__restrict__ bin,
                           const uint64_t *__restrict__ tile_mask) {
  // staged hits: the three bf16 terms of the six block-frame coefficients of log2(opacity * G) (exp_mfma.hpp), the
  // blended values (r, g, b, depth) for the recurrence, and what the moment step needs: (x - cx, y - cy, A, B), (C, opacity), id
  __shared__ uint4 q_k[3][kChunk];
  __shared__ float4 q_col[kChunk], q_t0[kChunk];
  __shared__ float2 q_t1[kChunk];
  __shared__ __attribute__((aligned(16))) uint32_t q_id[kChunk];
  // [row][pixel] matrix of one half-group (8 splats).  split form: rows 0..7 = first fp16 terms (v | w << 16) of the 8
  // splats, rows 8..15 = second terms; exact form: rows 0..7 = v, rows 8..15 = w (fp32)
  __shared__ __attribute__((aligned(16))) uint32_t xm[16 * kXStride];
  float *dbuf = reinterpret_cast<float *>(xm);   // split form: the 2 x 16 x 14 result tile reuses the matrix once the MFMAs have consumed it
  float *rbuf = reinterpret_cast<float *>(xm);   // a chunk's 64 result rows wait here between the chunk's last group and the next one's first
  float *xs = reinterpret_cast<float *>(xm);     // prologue scratch: 64 x 4 floats
  static_assert(2 * kGroup * kDStride <= 13 * kXStride && kChunk * kRStride <= 13 * kXStride && 64 * 4 <= 13 * kXStride,
                "scratch fits below the zero fragments");
  static_assert(kAccStride == 16 && kRStride >= 10 && kRStride % 4 == 0, "a result row's ten floats map onto an accumulator row lane for lane");
  static_assert(kXStride != 68 ||
                sizeof(uint4) * 3 * kChunk + sizeof(float4) * 2 * kChunk + sizeof(float2) * kChunk + 4 * kChunk + 4 * 16 * kXStride == 10240,
                "10 KiB of LDS per wave: four waves per SIMD fill the CU's 160 KiB exactly");
  const int lane = threadIdx.x;
  BlockWave blk;
  if (!block_wave(tiles, tiles_x, blk)) return;
  const int quad = blk.quad, bx = blk.bx, by = blk.by;
  const int px = bx + (lane & 7), py = by + (lane >> 3);
  const bool inside = px < W && py < H;
  const float cx = (float)bx + 3.5f, cy = (float)by + 3.5f;  // block-frame origin of the exponent's coefficients and of the moments
  // A operand of the exponent MFMAs: half of the lanes feed zeros (exp_mfma.hpp).  The zero fragments live in the four
  // padding dwords of rows 13..15 of the [row][pixel] matrix (nothing ever writes there: rows are written [row][lane])
  const uint4 basis = pixel_basis_frag(lane);
  const bool a_on = a_operand_active(lane);
  const int a_slot = a_operand_slot(lane);
  if (lane < 3) *reinterpret_cast<uint4 *>(&xm[(13 + lane) * kXStride + 64]) = make_uint4(0u, 0u, 0u, 0u);
  const TileRange tr = tile_range(tile_start, blk.tile, capacity);
  // deterministic mode: the sums leave as plain rows partial[4 * pair + quad], pair = the (Gaussian, tile) pair's ordinal
  // in GAUSSIAN-major order (pair_base[id] + the tile's rank in the Gaussian's tile mask), with a flag byte per row
  constexpr bool det = kDet;
  if (tr.end == tr.beg) return;
  const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
  // all of the pixel's loads are issued together (no load waits on `last`); pixels nothing was blended into drop
  // their upstream gradient afterwards by a select (it may be NaN: depth / alpha at empty pixels)
  float T_final = 0.0f, dpix0 = 0.0f, dpix1 = 0.0f, dpix2 = 0.0f, ddep = 0.0f, dalp = 0.0f;
  uint32_t last = 0u;
  if (inside) {
    T_final = final_T[pix];
    last = n_contrib[pix];
    dpix0 = dL_dcolor[pix]; dpix1 = dL_dcolor[HW + pix]; dpix2 = dL_dcolor[2 * HW + pix];
    if (kHasDA && dL_ddepth) ddep = dL_ddepth[pix];
    if (kHasDA && dL_dalpha) dalp = dL_dalpha[pix];
  }
  if (last == 0) { dpix0 = dpix1 = dpix2 = ddep = dalp = 0.0f; }
  const uint32_t todo = wave_max_u32(last);   // wave-uniform (SGPR): the chunk loop and the slot indices live in SGPRs
  if (todo == 0) return;
  // split form: one power-of-two scale per wave from the block's largest upstream gradient
  float sv = 1.0f, inv_sv = 1.0f;
  if constexpr (!kExact) {
    float amax = fmaxf(fmaxf(fabsf(dpix0), fabsf(dpix1)), fabsf(dpix2));
    if (kHasDA) amax = fmaxf(amax, fmaxf(fabsf(ddep), fabsf(dalp)));
    const int eb = (int)((wave_max_u32(__float_as_uint(amax)) >> 23) & 0xFFu);   // biased exponent (|x| orders like its bits); 0: zero / denormal
    int sb = eb == 0 ? 127 : 254 + (kHasDA ? kVTargetExpDA : kVTargetExp) - eb;   // biased exponent of the scale
    sb = min(max(sb, 1), 253);
    sv = __uint_as_float((uint32_t)sb << 23);
    inv_sv = __uint_as_float((uint32_t)(254 - sb) << 23);
  }
  // In the split form the recurrence runs on T' = 2^10 T (so that w' = alpha T' is the scaled blend weight at no cost)
  // and on upstream gradients scaled by sv / 2^10, which makes dL/dalpha come out scaled by sv:
  //   sv dL/dalpha = (s'' - R'') T' - (sv T_final bg.dL/dcolor) / (1 - alpha).
  const float tf_bg = sv * (T_final * (bg[0] * dpix0 + bg[1] * dpix1 + bg[2] * dpix2));
  const int bn = lane & 15, bk = lane >> 4;
  // Every lane already holds its own pixel's four gradients, so the B operand's W columns are exchanged through LDS
  // (the matrices are idle until the first group) instead of being gathered from global memory again.
  xs[lane * 4 + 0] = sv * dpix0; xs[lane * 4 + 1] = sv * dpix1; xs[lane * 4 + 2] = sv * dpix2; xs[lane * 4 + 3] = sv * ddep;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  // B operand.  A lane supplies ONE column bn of the 16-column basis: columns 0..5 are the position basis of the V half
  // (1, x, y, x^2, xy, y^2 in the block frame), the following ones the upstream gradients (dL/dr, dL/dg, dL/db,
  // dL/ddepth) of the W half.
  union Frag { f16x8 v; uint4 q; uint32_t d[4]; };
  // exact form: lane = 4 b + j of the 16-block 4x4x1 MFMA, block b = (quad qb of the half-group's hits, pixel row rb)
  const int jb = lane & 3, qb = (lane >> 2) & 1, rb = (lane >> 4) | ((lane >> 1) & 4);
  const float ylb = (float)rb - 3.5f;
  float bv[kExact ? 8 : 1], bw[kExact ? 8 : 1];
  Frag bh[kExact ? 1 : 4];
  if constexpr (kExact) {
#pragma unroll
    for (int k = 0; k < 8; k++) {   // fp32 MFMA k covers pixel (k, rb) of every block
      const float xl = (float)k - 3.5f;
      bv[k] = jb == 0 ? 1.0f : jb == 1 ? xl : jb == 2 ? xl * xl : ylb;
      bw[k] = xs[(8 * rb + k) * 4 + jb];
    }
  } else {
    // fp16 MFMA m covers pixels 16 bk + 4 m + j, j = 0..3: element 2j = v slot, 2j + 1 = w slot.  V columns (bn < 6) come
    // from the constant table (two 16-byte loads per lane), W columns from the exchanged gradients.
    uint4 tv[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    if (bn < 6) {
      const uint4 *tp = reinterpret_cast<const uint4 *>(&kBasisV.v[bn][16 * bk]);
      tv[0] = tp[0]; tv[1] = tp[1];
    }
    const uint32_t tw[8] = {tv[0].x, tv[0].y, tv[0].z, tv[0].w, tv[1].x, tv[1].y, tv[1].z, tv[1].w};
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int q = 16 * bk + 4 * m + j, e = 4 * m + j;
        const uint32_t vbits = (e & 1) ? tw[e >> 1] >> 16 : tw[e >> 1] & 0xFFFFu;
        const float g = (bn >= 6 && bn <= 13) ? xs[q * 4 + ((bn - 6) & 3)] : 0.0f;
        const uint32_t g1 = pack_rtz16(g, 0.0f);
        const float gw = bn <= 9 ? half_lo(g1) : g - half_lo(g1);     // columns 6..9: first term, 10..13: the remainder
        bh[m].d[j] = vbits | (pack_rtz16(gw, 0.0f) << 16);
      }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if constexpr (!kExact) {
    const float sq = sv * (1.0f / kWScale);
    dpix0 *= sq; dpix1 *= sq; dpix2 *= sq; ddep *= sq; dalp *= sq;
  }
  float T = kExact ? T_final : kWScale * T_final, R = 0.0f, s_last = 0.0f, last_alpha = 0.0f;
  const int abase = kExact ? (4 * qb + jb) * kXStride + 8 * rb : (lane & 15) * kXStride + 16 * (lane >> 4);
  constexpr int kAStep = 4;   // dwords between the lane's four 16-byte reads
  // exact form, the sums over the block's rows: rows rb and rb ^ 2 meet in a permlane32 swap (lane bit 5), whose two outputs
  // hold the rows with rb bit 1 clear (y = yl_lo) / set (y = yl_lo + 2)
  const float yl_lo = (float)(rb & 5) - 3.5f;
  // A chunk's results wait in LDS as 64 rows of kRStride floats (`rbuf`, written by convert_chunk) with the rows' ids still in
  // q_id; `nflush` = the number of rows waiting (wave-uniform).  flush_rows sends them off: up to sixteen wave-wide atomic
  // instructions (lane = float of a 64-byte accumulator row, four rows per instruction, ten lanes of sixteen active: one
  // memory-side request per splat; zero terms are skipped).  It is called behind the issue of the NEXT chunk's gathers and
  // in front of the staging stores that overwrite q_id: vmcnt counts loads and atomics alike and the compiler waits with
  // vmcnt(0) for the gathers, so atomics issued at the end of the chunk would be waited for, at their full memory-side
  // latency, at the top of the next one.  Offsets: N * 16 < 2^32 floats (checked at the entry point).
  // det: the rows are written whole to partial[4 * pair + quad] (zeros included: nothing was cleared beforehand), q_id
  // holds the pair ordinal
  int nflush = 0;
  auto flush_rows = [&]() {
    const int col = lane & 15, r4 = lane >> 4;
    const float *rp = rbuf + r4 * kRStride + col;
    const uint32_t *ip = q_id + r4;
    const bool used = kColorOnly ? (col >= 6 && col < 9) : col < 10;
    // the rows' values and ids are fetched together (one LDS round trip for the burst, not two per instruction); the addresses
    // are in bounds for every lane, rows beyond the chunk and unused columns are masked afterwards
#ifndef SCORP_BWD_FLUSH_BATCH
#define SCORP_BWD_FLUSH_BATCH 16
#endif
    constexpr int kBatch = SCORP_BWD_FLUSH_BATCH;   // atomic instructions per LDS round trip
#pragma unroll
    for (int k0 = 0; k0 < kChunk / 4; k0 += kBatch) {
      if (4 * k0 < nflush) {   // wave-uniform
        float val[kBatch];
        uint32_t rid[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; j++) {
          val[j] = rp[4 * (k0 + j) * kRStride];
          rid[j] = ip[4 * (k0 + j)];
        }
#pragma unroll
        for (int j = 0; j < kBatch; j++) asm volatile("" : "+v"(val[j]), "+v"(rid[j]));   // (the reads stay in front of the branches)
#pragma unroll
        for (int j = 0; j < kBatch; j++) {
          const bool row = r4 < nflush - 4 * (k0 + j);
          if (det) {
            const uint32_t pair = row ? rid[j] : 0xFFFFFFFFu;
            if (pair < capacity && col < 10) {   // (an ordinal beyond the reservation: an overflowed view, discarded anyway)
              partial[(pair * 4u + (uint32_t)quad) * (uint32_t)kAccStride + col] = used ? val[j] : 0.0f;
              if (col == 0) row_flags[pair * 4u + (uint32_t)quad] = 1;
            }
          } else if (row && used && val[j] != 0.0f) {
            atomicAdd(acc + (rid[j] * (uint32_t)kAccStride + col), val[j]);
          }
        }
      }
    }
    nflush = 0;
  };
  // slots of a group: head + i, head a multiple of kGroup: one LDS base per array, immediate offsets.  `top` = 1-based
  // position in the hit list of the group's first slot (positions fall by one per slot).
  // A group is two halves of 8 splats.  Each half: 1a, 1b, then ONE pass over the matrix pipe whose 16 rows are
  // (8 slots) x (first term | second term) [exact form: (8 slots) x (v | w)], so the [row][pixel] matrix in LDS is
  // 16 x 64 dwords whatever the form; the two halves' results wait in registers and leave together.
  auto process_group = [&](auto full, auto clampy, int nslots, int head, int top) {
    constexpr bool kFull = decltype(full)::value;   // full groups run straight-line; only a wave's last one is partial
    constexpr bool kClamp = decltype(clampy)::value;   // the chunk holds a splat with opacity > 0.99 (the forward's rule:
                                                       // only such a splat can reach alpha = 0.99; the others skip the v_min)
    int hv = head;
    asm volatile("" : "+v"(hv));   // keep the group's LDS bases in VGPRs (else every ds_read re-moves an SGPR base)
    const float4 *gcol = q_col + hv;
    const int first = top - (int)last;   // slot i takes part in this pixel's blend iff top - i <= last, i.e. i >= first
    // log2(opacity * G) of the group's 16 hits at this lane's pixel: three MFMAs (the forward's, bit for bit)
    const uint4 *ka0 = a_on ? &q_k[0][hv + a_slot] : reinterpret_cast<const uint4 *>(&xm[13 * kXStride + 64]);
    const uint4 *ka1 = a_on ? &q_k[1][hv + a_slot] : reinterpret_cast<const uint4 *>(&xm[14 * kXStride + 64]);
    const uint4 *ka2 = a_on ? &q_k[2][hv + a_slot] : reinterpret_cast<const uint4 *>(&xm[15 * kXStride + 64]);
    const f32x16 ev = block_exponents(*ka0, *ka1, *ka2, basis);
    f32x4 dd[kExact ? 1 : 2] = {};
#pragma unroll
    for (int h = 0; h < 2; h++) {
      if (kFull || h * 8 < nslots) {   // wave-uniform
        // One straight-line pass per splat (alpha, then the recurrence): with four waves per SIMD an in-order wave's own
        // issue interval already covers the ALU latencies, so nothing is gained by separating a parallel alpha phase
        // from the sequential part - and keeping eight (alpha, record) sets live costs the registers that let the
        // staged records of the NEXT splats be fetched from LDS ahead of their use.
        // The staged records are fetched kAhead splats ahead of their use (explicit rotation: left alone the scheduler
        // issues each ds_read right in front of its use and the wave eats the LDS latency once per splat).
#ifndef SCORP_BWD_AHEAD
#define SCORP_BWD_AHEAD 3
#endif
        constexpr int kAhead = SCORP_BWD_AHEAD;
        float4 rc[kAhead];
#pragma unroll
        for (int j = 0; j < kAhead - 1; j++) rc[j] = gcol[h * 8 + j];
#pragma unroll
        for (int i8 = 0; i8 < 8; i8++) {
          const int i = h * 8 + i8;
          if (i8 + kAhead - 1 < 8) rc[(i8 + kAhead - 1) % kAhead] = gcol[i + kAhead - 1];
          if (kFull || i < nslots) {  // wave-uniform: stale staging entries beyond the group must not enter the recurrence
            const float4 col = rc[i8 % kAhead];   // r, g, b, depth
            const float g_o = __builtin_amdgcn_exp2f(ev[i]);
            // alpha = min(0.99, g_o) >= 1/255  <=>  g_o >= 1/255
            bool ok = (i >= first) & (g_o >= kAlphaMin);
            if constexpr (kClamp) ok = ok & (g_o <= guard_limit_unpack(q_k[0][hv + i].w));   // the forward's `power > 0` skip
            const float Go = ok ? g_o : 0.0f;
            const float alpha = kClamp ? fminf(kAlphaMax, Go) : Go;
            const float rinv = __builtin_amdgcn_rcpf(1.0f - alpha);
            T *= rinv;
            const float w = alpha * T;
            float v = 0.0f;
            if constexpr (!kColorOnly) {
              R = last_alpha * (s_last - R) + R;
              const float sc = kHasDA ? col.x * dpix0 + col.y * dpix1 + col.z * dpix2 + col.w * ddep + dalp
                                      : col.x * dpix0 + col.y * dpix1 + col.z * dpix2;
              const float dL_dal = (sc - R) * T - tf_bg * rinv;
              s_last = sc;
              last_alpha = alpha;
              v = Go * dL_dal;
            }
            if constexpr (kExact) {
              xm[i8 * kXStride + lane] = __float_as_uint(v);
              xm[(8 + i8) * kXStride + lane] = __float_as_uint(w);
            } else if constexpr (kColorOnly) {
              const uint32_t p1 = pack_rtz16(0.0f, w);
              xm[i8 * kXStride + lane] = p1;
              xm[(8 + i8) * kXStride + lane] = pack_rtz16(0.0f, __builtin_fmaf(half_hi(p1), -1.0f, w));
            } else {   // x = h1 + h2, two fp16 terms (round toward zero, saturating); v and w share the dwords
              const uint32_t p1 = pack_rtz16(v, w);
              const uint32_t p2 = pack_rtz16(__builtin_fmaf(half_lo(p1), -1.0f, v), __builtin_fmaf(half_hi(p1), -1.0f, w));
              xm[i8 * kXStride + lane] = p1;
              xm[(8 + i8) * kXStride + lane] = p2;
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // A operands: the lane's 16 pixels are consecutive in its row, fetched as four 16-byte reads issued together
        f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (kExact) {
          // block (qb, rb), MFMA k: A = v (then w) of hit 4 qb + i at pixel (k, rb), B = column jb at that pixel.  The lane's
          // eight pixels are its row's two 16-byte runs in the v rows and the same two in the w rows.
          float av[16];
#pragma unroll
          for (int t4 = 0; t4 < 4; t4++)
            *reinterpret_cast<float4 *>(&av[4 * t4]) =
                *reinterpret_cast<const float4 *>(&xm[abase + (t4 >> 1) * 8 * kXStride + kAStep * (t4 & 1)]);
          f32x4 dw = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int k = 0; k < 8; k++) d = __builtin_amdgcn_mfma_f32_4x4x1f32(av[k], bv[k], d, 0, 0, 0);
#pragma unroll
          for (int k = 0; k < 8; k++) dw = __builtin_amdgcn_mfma_f32_4x4x1f32(av[8 + k], bw[k], dw, 0, 0, 0);
          // d[i] / dw[i] at lane (jb, qb, rb): row rb's sum of column jb for hit 4 qb + i.  Sum over the eight rows: lane bit 5
          // (permlane32 swap), bit 4 (permlane16 swap) - each swap pairs two registers, so the register count halves
          // per step - and bit 3 (DPP).  y-weighted sums (Q) ride along: column 1 gives sum y x v, column 3 (= y) sum y^2 v.
          // swap32: lo = (a | b) of lanes 0..31 in lanes (0..31 | 32..63), hi = the same of lanes 32..63: the rows with rb
          // bit 1 clear / set; lo + hi is a's row sum in lanes 0..31 and b's in lanes 32..63
          auto swap32 = [](float a, float b, float &lo, float &hi) {
            const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
            lo = __uint_as_float(s[0]); hi = __uint_as_float(s[1]);
          };
          auto sum16 = [](float a, float b) {
            const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
            return __uint_as_float(s[0]) + __uint_as_float(s[1]);
          };
          float l0, h0, l1, h1, l2, h2, l3, h3;
          swap32(d[0], d[1], l0, h0); swap32(d[2], d[3], l1, h1);
          swap32(dw[0], dw[1], l2, h2); swap32(dw[2], dw[3], l3, h3);
          const float s0 = l0 + h0, s1 = l1 + h1;
          float p = sum16(s0, s1);
          float qy = sum16(__builtin_fmaf(yl_lo, s0, h0 + h0), __builtin_fmaf(yl_lo, s1, h1 + h1));   // y = yl_lo (+ 2 in h)
          float rw = sum16(l2 + h2, l3 + h3);
          p += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(p), 0x128, 0xF, 0xF, true));     // row_ror:8
          qy += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(qy), 0x128, 0xF, 0xF, true));
          rw += __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(rw), 0x128, 0xF, 0xF, true));
          asm volatile("" : "+v"(p), "+v"(qy), "+v"(rw));   // (the adds stay in front of the branch: one v_add_f32_dpp each)
          // hit 4 qb + 2 (lane bit 4) + (lane bit 5), column jb.  The slot's three float4 (sum v {1, x, x^2, y}, sum y v {1, x,
          // x^2, y}, sum w {dL/dr, dL/dg, dL/db, dL/ddepth}) go to q_k[1], q_k[2] and q_col of the slot: the group's exponents
          // and this half's recurrence are done with them, and the matrix is still needed by the next half
          if (!(lane & 8)) {
            const int sl = hv + h * 8 + 4 * qb + 2 * ((lane >> 4) & 1) + (lane >> 5);
            reinterpret_cast<float *>(&q_k[1][sl])[jb] = p;
            reinterpret_cast<float *>(&q_k[2][sl])[jb] = qy;
            reinterpret_cast<float *>(&q_col[sl])[jb] = rw;
          }
        } else {
          Frag af[4];
#pragma unroll
          for (int m = 0; m < 4; m++) af[m].q = *reinterpret_cast<const uint4 *>(&xm[abase + kAStep * m]);
#pragma unroll
          for (int m = 0; m < 4; m++) d = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[m].v, bh[m].v, d, 0, 0, 0);
        }
        if constexpr (!kExact) dd[h] = d;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();   // the next half (and the result tile) overwrite the matrix
      }
    }
    // split form: result tile [term][slot][column] (it reuses the matrix): lane (bn, bk) holds rows 4 bk .. 4 bk + 3 of column
    // bn.  Sixteen lanes add the two terms and leave the slot's ten block-frame moments in the slot's own staging entries,
    // laid out like the exact form's sums (the group is done with them): one tail serves every form (convert_chunk)
    if constexpr (!kExact) {
      if (bn < 14) {
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
          for (int r = 0; r < 4; r++)
            dbuf[((bk >> 1) * kGroup + h * 8 + ((4 * bk + r) & 7)) * kDStride + bn] = dd[h][r];
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (lane < nslots) {
        const float *m = dbuf + lane * kDStride;
        const float *m2 = m + kGroup * kDStride;
        const float4 u0 = *reinterpret_cast<const float4 *>(m), u1 = *reinterpret_cast<const float4 *>(m + 4),
                     u2 = *reinterpret_cast<const float4 *>(m + 8), u3 = *reinterpret_cast<const float4 *>(m + 12);
        const float4 w0 = *reinterpret_cast<const float4 *>(m2), w1 = *reinterpret_cast<const float4 *>(m2 + 4),
                     w2 = *reinterpret_cast<const float4 *>(m2 + 8), w3 = *reinterpret_cast<const float4 *>(m2 + 12);
        // first + second term; W sums = (first-term + remainder columns) of the upstream gradients
        const float inv_w = inv_sv * (1.0f / kWScale);
        float mm[10];
        mm[0] = (u0.x + w0.x) * inv_sv; mm[1] = (u0.y + w0.y) * inv_sv; mm[2] = (u0.z + w0.z) * inv_sv;
        mm[3] = (u0.w + w0.w) * inv_sv; mm[4] = (u1.x + w1.x) * inv_sv; mm[5] = (u1.y + w1.y) * inv_sv;
        mm[6] = ((u1.z + w1.z) + (u2.z + w2.z)) * inv_w; mm[7] = ((u1.w + w1.w) + (u2.w + w2.w)) * inv_w;
        mm[8] = ((u2.x + w2.x) + (u3.x + w3.x)) * inv_w; mm[9] = ((u2.y + w2.y) + (u3.y + w3.y)) * inv_w;
        if constexpr (!kColorOnly) {
          *reinterpret_cast<float4 *>(&q_k[1][hv + lane]) = make_float4(mm[0], mm[1], mm[3], mm[2]);
          *reinterpret_cast<float4 *>(&q_k[2][hv + lane]) = make_float4(0.0f, mm[4], 0.0f, mm[5]);
        }
        q_col[hv + lane] = make_float4(mm[6], mm[7], mm[8], mm[9]);
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();   // (the next group overwrites the result tile)
    }
  };
  // The chunk's tail, once per 64 hits with every lane holding a slot: the slot's block-frame moments (sum v {1, x, x^2, y},
  // sum y v {., x, ., y}, sum w {dL/dr, dL/dg, dL/db, dL/ddepth} in its three staging entries) -> its ten screen-space
  // gradients, left as row `lane` of rbuf for flush_rows.  The matrix is idle between chunks; 64 rows of kRStride floats end
  // below the zero fragments of its rows 13..15.
  auto convert_chunk = [&](int n) {
    if (lane < n) {
      const float4 a = q_t0[lane];     // x - cx, y - cy, A, B
      const float2 b = q_t1[lane];     // C, opacity
      const float opac = b.y;
      const float cA = a.z * (-1.0f / kConicScale), cB = a.w * (-0.5f / kConicScale), cC = b.x * (-1.0f / kConicScale);
      const float xl = a.x, yl = a.y;
      float *m = rbuf + lane * kRStride;
      const float4 u2 = q_col[lane];
      if constexpr (kColorOnly) {
        *reinterpret_cast<float4 *>(m) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        *reinterpret_cast<float4 *>(m + 4) = make_float4(0.0f, 0.0f, u2.x, u2.y);
        *reinterpret_cast<float2 *>(m + 8) = make_float2(u2.z, 0.0f);
      } else {
        const float4 u0 = *reinterpret_cast<const float4 *>(&q_k[1][lane]), u1 = *reinterpret_cast<const float4 *>(&q_k[2][lane]);
        const float m0 = u0.x, mx = u0.y, my = u0.w, mxx = u0.z, mxy = u1.y, myy = u1.w;
        const float svdx = xl * m0 - mx, svdy = yl * m0 - my;
        const float svdx2 = xl * xl * m0 - 2.0f * xl * mx + mxx;
        const float svdxdy = xl * yl * m0 - xl * my - yl * mx + mxy;
        const float svdy2 = yl * yl * m0 - 2.0f * yl * my + myy;
        *reinterpret_cast<float4 *>(m) = make_float4(0.5f * W * (-cA * svdx - cB * svdy), 0.5f * H * (-cC * svdy - cB * svdx),
                                                     -0.5f * svdx2, -svdxdy);
        *reinterpret_cast<float4 *>(m + 4) = make_float4(-0.5f * svdy2, m0 / opac, u2.x, u2.y);
        *reinterpret_cast<float2 *>(m + 8) = make_float2(u2.z, u2.w);
      }
    }
    nflush = n;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };

  // The chunk's gathers are a chain of dependent loads (hit-list entry -> record) of ~1 us each way; with three waves
  // per SIMD nothing hides them, so they are software-pipelined two chunks deep: while chunk c is replayed the records
  // of chunk c+1 and the list entries of chunk c+2 are already in flight.  Chunk c holds the hits at 0-based positions
  // todo - 64 c - 1 (slot 0) down to todo - 64 c - 64 (slot 63): slots ascend back to front.
  const uint32_t *my_hits = block_hit_list(hits, quad, capacity, tr.beg);
  auto fetch_id = [&](uint32_t c_) {
    const int o = (int)todo - (int)(kChunk * c_) - 1 - lane;
    return o >= 0 ? my_hits[o] : 0xFFFFFFFFu;
  };
  auto fetch_rec = [&](uint32_t id_, float4 &a_, float4 &b_, float4 &c_) {
    if (id_ != 0xFFFFFFFFu) {
      const float4 *src = reinterpret_cast<const float4 *>(rec + id_);
      a_ = src[0]; b_ = src[1]; c_ = src[2];
    }
  };
  float4 a, b, c;
  uint32_t id = fetch_id(0);
  fetch_rec(id, a, b, c);
  uint32_t id1 = fetch_id(1);
  const uint32_t nchunks = (todo + kChunk - 1) / kChunk;
  for (uint32_t ch = 0; ch < nchunks; ch++) {
    float4 a1, b1, c1;
    fetch_rec(id1, a1, b1, c1);
    const uint32_t id2 = fetch_id(ch + 2);
    flush_rows();   // the previous chunk's rows: behind the issue of this chunk's gathers, in front of the staging stores
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (id != 0xFFFFFFFFu) {
      uint4 k0, k1, k2;
      splat_block_coefs(a.x, a.y, a.z, a.w, b.x, b.y, cx, cy, k0, k1, k2);
      k0.w = guard_limit_pack(c.w);   // the forward's bits (exp_mfma.hpp)
      q_k[0][lane] = k0; q_k[1][lane] = k1; q_k[2][lane] = k2;
      q_col[lane] = make_float4(b.z, b.w, c.x, c.y);
      q_t0[lane] = make_float4(a.x - cx, a.y - cy, a.z, a.w);
      q_t1[lane] = make_float2(b.x, c.w);
      if constexpr (det) {
        // the (Gaussian, tile) pair's ordinal, Gaussian-major (pair_rank)
        const uint4 raw = reinterpret_cast<const uint4 *>(bin)[id];
        const BinRec br = *reinterpret_cast<const BinRec *>(&raw);
        const uint64_t mk = tile_mask[id];
        q_id[lane] = pair_base[id] + pair_rank(br, mk, blk.tx, blk.ty);
      } else {
        q_id[lane] = id;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int top = (int)todo - (int)(kChunk * ch);          // 1-based position of slot 0
    const int n = top < kChunk ? top : kChunk;               // hits in this chunk (only the last chunk is short)
    // (b.y = log2(opacity); an indefinite conic takes the same instantiation for its `power > 0` guard)
    const bool hot = __ballot(id != 0xFFFFFFFFu && (b.y > kLog2AlphaMax - 1e-4f || rec_is_indefinite(c.z))) != 0;
    for (int head = 0; head < n; head += kGroup) {
      if (n - head < kGroup) process_group(std::false_type{}, std::true_type{}, n - head, head, top - head);
      else if (hot) process_group(std::true_type{}, std::true_type{}, kGroup, head, top - head);
      else process_group(std::true_type{}, std::false_type{}, kGroup, head, top - head);
    }
    convert_chunk(n);
    id = id1; a = a1; b = b1; c = c1; id1 = id2;
  }
  flush_rows();
}
}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_gs3d_backward_scratch_bytes_ex(int32_t N, int32_t W, int32_t H, uint64_t capacity, uint32_t flags) {
  (void)W; (void)H;
  return backward_scratch_bytes(N, capacity, flags, kAccStride) + sh_jacobian_bytes(N);
}

extern "C" size_t scorp_gs3d_backward_scratch_bytes(int32_t N) {
  return backward_scratch_bytes(N, 0, 0u, kAccStride) + sh_jacobian_bytes(N);
}

extern "C" int scorp_gs3d_backward(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                                   const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                                   const ScorpGs3dGrads *grads, void *scratch, size_t scratch_bytes,
                                   scorp_stream_t stream_) {
  return scorp_gs3d_backward_ex(in, state, pairs, capacity, dL_dcolor, dL_ddepth, dL_dalpha, grads, scratch, scratch_bytes,
                                0u, stream_);
}

extern "C" int scorp_gs3d_backward_ex(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                                      const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                                      const ScorpGs3dGrads *grads, void *scratch, size_t scratch_bytes, uint32_t flags,
                                      scorp_stream_t stream_) {
  return backward3d_impl(in, state, pairs, capacity, dL_dcolor, dL_ddepth, dL_dalpha, grads, scratch, scratch_bytes, flags, stream_,
                         nullptr);
}

// `adam` (scorp_gs3d_train_view): the per-Gaussian kernel applies the optimizer step and the view's statistics itself
int scorp::backward3d_impl(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                           const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                           const ScorpGs3dGrads *grads, void *scratch, size_t scratch_bytes, uint32_t flags,
                           scorp_stream_t stream_, const AdamEpi *adam, float lambda_isotropic, const float *jac) {
  hipStream_t stream = (hipStream_t)stream_;
  const char *base = (const char *)state, *pb = (const char *)pairs;
  auto blend = [&](const StateLayout &L, const PairLayout &P, float *acc, float *partial, uint8_t *row_flags, uint32_t *pair_base) {
    const int blocks = block_wave_grid(L.tiles);
    const bool det = partial != nullptr, da = dL_ddepth || dL_dalpha, exact = (flags & SCORP_BACKWARD_EXACT_FP32) != 0;
    // nothing but colour gradients wanted (every geometry / opacity output NULL): the colour-only replay
    const bool adam_geom = adam && adam->on && (adam->m[0] || adam->m[3] || adam->m[4] || adam->m[5] || adam->accum);
    const bool color_only = !exact && !adam_geom && !grads->means3D && !grads->means2D && !grads->opacities && !grads->scales &&
                            !grads->rotations && !grads->cov3D_precomp;
    auto wk = det ? (color_only ? blend_backward_wave_kernel<false, false, true, true>
                     : exact ? (da ? blend_backward_wave_kernel<true, true, false, true> : blend_backward_wave_kernel<false, true, false, true>)
                             : (da ? blend_backward_wave_kernel<true, false, false, true> : blend_backward_wave_kernel<false, false, false, true>))
              : color_only ? blend_backward_wave_kernel<false, false, true>
              : exact ? (da ? blend_backward_wave_kernel<true, true> : blend_backward_wave_kernel<false, true>)
                      : (da ? blend_backward_wave_kernel<true, false> : blend_backward_wave_kernel<false, false>);
    wk<<<blocks, 64, 0, stream>>>(
        (const uint32_t *)(base + L.tile_start), (const uint32_t *)(pb + P.hits), (const SplatRec *)(base + L.rec),
        (uint32_t)capacity, in->image_width, in->image_height, L.tiles_x, L.tiles, in->bg, (const float *)(base + L.final_T),
        (const uint32_t *)(base + L.n_contrib), dL_dcolor, dL_ddepth, dL_dalpha, acc, partial, row_flags, pair_base,
        (const BinRec *)(base + L.bin), (const uint64_t *)(base + L.tile_mask));
  };
  auto per_gaussian = [&](const StateLayout &L, const float *acc) {
    launch_preprocess_backward(in, L, (const BinRec *)(base + L.bin), acc, grads, stream, adam, lambda_isotropic, jac);
  };
  return backward_pass(kGs3d, in, state, pairs, capacity, dL_dcolor, grads, scratch, scratch_bytes, flags, stream, blend,
                       per_gaussian);
}
