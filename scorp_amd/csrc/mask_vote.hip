// mask_vote.hip — 3-D segmentation by 2-D object masks: per Gaussian and object, the blend weight a render put inside
// the object's mask and outside it, in one front-to-back replay of the hit lists the render left for the backward.
//
// Replaces the vote of utils/mask.py:42-124 (get_mask3d): there each object costs two full backward passes with
// colors_precomp = ones, and only |dL/dcolor| of each Gaussian is read.  With w_i(p) = alpha_i(p) T_i(p) the blend weight
// the render gave Gaussian i at pixel p, that norm is S_in / (sqrt(3) H W) for the loss mean(render * mask), where
//     S_in[k, i] = sum over the pixels of mask k of w_i(p),    S_out[k, i] = the same sum over the pixels outside it.
// This file computes S_in and S_out directly.
//
// One wave per 8x8 pixel block, numbered as the blend kernels number theirs.  The wave walks its block's HIT LIST front to
// back (the splat ids that passed the exact block test, left by scorp_gs3d_render / scorp_gs2d_render in the pair buffer),
// up to the deepest last contributor of its pixels (n_contrib).  Alpha is recomputed with the forward's own arithmetic -
// 3DGS: the exponent MFMAs of exp_mfma.hpp on the block-frame coefficients; 2DGS: surfel_lin / eval_surfel of
// surfel.hpp - and the transmittance runs front to back as the forward runs it, so w is the forward's w bit for bit and a
// hit contributes to a pixel iff its position is at most the pixel's last contributor and alpha >= 1/255 (the forward's
// termination rule is already in n_contrib).
//
// The reduction over the block's 64 pixels runs on the matrix cores: D[16 hits][16 columns] = W[16 hits][64 pixels] x
// B[64 pixels][16 columns], B[p] = (m_0, 1 - m_0, ..., m_7, 1 - m_7) for the eight objects of the pass.  The masks are 0 / 1,
// so W stays fp32 and the products are exact: sixteen v_mfma_f32_16x16x4_f32 per group of 16 hits.  No float atomics:
// every (block, hit) leaves its 16 sums as one plain 64-byte row at the Gaussian-major ordinal of its (Gaussian, tile) pair
// (the deterministic backward's layout), and reduce_pair_rows_kernel adds each Gaussian's rows in a fixed order.  The
// epilogue applies the method and ADDS into the caller's output, so views accumulate without extra launches.  Two runs
// give the same bits: the vote reads signs.
#include "common.hpp"
#include "exp_mfma.hpp"
#include "surfel.hpp"

namespace scorp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kVChunk = 64;          // hits staged per chunk (one per lane)
constexpr int kVGroup = 16;          // hits per MFMA group
constexpr int kVStride = 68;         // dwords per hit row of the [hit][pixel] weight matrix (16-byte aligned rows)
constexpr int kVoteObjects = 8;      // objects per pass: columns (m_k, 1 - m_k)
constexpr int kVoteRow = 16;         // floats per partial row (64 bytes)
#ifndef SCORP_VOTE_WAVES
#define SCORP_VOTE_WAVES 4
#endif

// k2d: the 2DGS state (Surfel records, ray-surfel intersection); otherwise the 3DGS one (SplatRec, exponent MFMAs)
template <bool k2d>
__global__ void __launch_bounds__(64, SCORP_VOTE_WAVES)
mask_vote_wave_kernel(const uint32_t *__restrict__ tile_start, const uint32_t *__restrict__ hits, const void *__restrict__ records,
                      uint32_t capacity, int W, int H, int tiles_x, int tiles, const uint32_t *__restrict__ n_contrib,
                      const uint8_t *__restrict__ masks, int num_masks, int k0, float *__restrict__ partial,
                      uint8_t *__restrict__ row_flags, const uint32_t *__restrict__ pair_base, const BinRec *__restrict__ bin,
                      const uint64_t *__restrict__ tile_mask) {
  // staged hits: 3DGS the three bf16 terms of the six block-frame coefficients (+ the guard limit); 2DGS the linear form of
  // the intersection.  q_id: the row of the hit's (Gaussian, tile) pair.
  __shared__ uint4 q_s[4][kVChunk];
  __shared__ uint32_t q_id[kVChunk];
  __shared__ __attribute__((aligned(16))) float xm[kVGroup * kVStride];
  __shared__ uint32_t q_mask[64];
  const int lane = threadIdx.x;
  BlockWave blk;
  if (!block_wave(tiles, tiles_x, blk)) return;
  const int quad = blk.quad, bx = blk.bx, by = blk.by;
  const int px = bx + (lane & 7), py = by + (lane >> 3);
  const bool inside = px < W && py < H;
  const float cx = (float)bx + 3.5f, cy = (float)by + 3.5f;
  const TileRange tr = tile_range(tile_start, blk.tile, capacity);
  if (tr.end == tr.beg) return;
  const size_t HW = (size_t)H * W, pix = (size_t)py * W + px;
  uint32_t last = 0u, mbits = 0u;   // mbits: bit j = pixel inside mask k0 + j
  if (inside) {
    last = n_contrib[pix];
    for (int j = 0; j < kVoteObjects && k0 + j < num_masks; j++) mbits |= (masks[(size_t)(k0 + j) * HW + pix] != 0 ? 1u : 0u) << j;
  }
  const uint32_t todo = min(wave_max_u32(last), tr.end - tr.beg);   // (wave-uniform; a hit list never outgrows its tile's list)
  if (todo == 0) return;
  // B operand.  fp32 MFMA t covers the pixels q = t + 16 bk (K index bk = lane >> 4); lane column bn = lane & 15 is object
  // k0 + bn / 2, inside (even bn) or outside (odd bn) its mask.  Objects beyond num_masks get zero columns.
  const int bn = lane & 15, bk = lane >> 4;
  q_mask[lane] = mbits;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float bb[16];
  {
    const bool obj = k0 + (bn >> 1) < num_masks;
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const uint32_t in_m = (q_mask[t + 16 * bk] >> (bn >> 1)) & 1u;
      bb[t] = obj ? (float)((bn & 1) ? 1u - in_m : in_m) : 0.0f;
    }
  }
  const uint4 basis = pixel_basis_frag(lane);   // 3DGS: the lane's monomials for the exponent MFMAs (exp_mfma.hpp)
  const bool a_on = a_operand_active(lane);
  const int a_slot = a_operand_slot(lane);
  const float qxb = (float)(lane & 7) - 3.5f, qyb = (float)(lane >> 3) - 3.5f, pxf = (float)px, pyf = (float)py;
  float T = 1.0f;
  const int abase = (lane & 15) * kVStride + 16 * bk;
  const uint32_t *my_hits = block_hit_list(hits, quad, capacity, tr.beg);
  const SplatRec *rec3 = reinterpret_cast<const SplatRec *>(records);
  const Surfel *rec2 = reinterpret_cast<const Surfel *>(records);

  // one group of up to 16 staged hits at slots head .. head + nslots - 1, 1-based list position of slot 0: pos0
  auto process_group = [&](int nslots, int head, uint32_t pos0) {
    int hv = head;
    asm volatile("" : "+v"(hv));
    f32x16 ev;
    if constexpr (!k2d) {
      uint4 a0 = q_s[0][hv + a_slot], a1 = q_s[1][hv + a_slot], a2 = q_s[2][hv + a_slot];
      if (!a_on) a0 = a1 = a2 = make_uint4(0u, 0u, 0u, 0u);   // (the other half of the lanes feeds zeros: exp_mfma.hpp)
      ev = block_exponents(a0, a1, a2, basis);
    }
#pragma unroll
    for (int i = 0; i < kVGroup; i++) {
      float w = 0.0f;
      if (i < nslots) {   // wave-uniform
        const bool listed = pos0 + (uint32_t)i <= last;
        if constexpr (k2d) {
          Eval2 h;
          const uint4 u0 = q_s[0][hv + i], u1 = q_s[1][hv + i], u2 = q_s[2][hv + i], u3 = q_s[3][hv + i];
          const bool ok = eval_surfel(*reinterpret_cast<const float4 *>(&u0), *reinterpret_cast<const float4 *>(&u1),
                                      *reinterpret_cast<const float4 *>(&u2), *reinterpret_cast<const float4 *>(&u3), qxb, qyb,
                                      pxf, pyf, h);
          const float al = (ok & listed) ? h.alpha : 0.0f;
          // the forward's order of operations (blend2d_forward_wave_kernel): test_T = T (1 - alpha), w = alpha T
          const float test_T = T * (1.0f - al);
          w = al * T;
          T = test_T;
        } else {
          const float g_o = __builtin_amdgcn_exp2f(ev[i]);
          // (the clamped form for every hit: for a splat that cannot reach 0.99 and has a definite conic the min and the
          // guard change no bit - the forward's clamp-free groups rely on the same fact)
          const bool live = listed & (g_o >= kAlphaMin) & (g_o <= guard_limit_unpack(q_s[0][hv + i].w));
          const float al = live ? fminf(kAlphaMax, g_o) : 0.0f;
          // the forward's order of operations (blend_forward_wave_kernel): test_T = fma(-alpha, T, T), w = alpha T
          const float test_T = __builtin_fmaf(-al, T, T);
          w = al * T;
          T = test_T;
        }
      }
      xm[i * kVStride + lane] = w;   // (slots beyond the group: zero rows)
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
    float4 av[4];
#pragma unroll
    for (int t4 = 0; t4 < 4; t4++) av[t4] = *reinterpret_cast<const float4 *>(&xm[abase + 4 * t4]);
#pragma unroll
    for (int t4 = 0; t4 < 4; t4++) {
      d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t4].x, bb[4 * t4], d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t4].y, bb[4 * t4 + 1], d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t4].z, bb[4 * t4 + 2], d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t4].w, bb[4 * t4 + 3], d, 0, 0, 0);
    }
    // lane (bn, bk) holds column bn of hits 4 bk .. 4 bk + 3: sixteen lanes write one 64-byte row
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int sl = 4 * bk + r;
      const uint32_t pair = sl < nslots ? q_id[hv + sl] : 0xFFFFFFFFu;
      if (pair < capacity) {
        const size_t row = (size_t)pair * 4u + (uint32_t)quad;
        partial[row * kVoteRow + bn] = d[r];
        if (bn == 0) row_flags[row] = 1;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the next group overwrites the matrix
  };

  // gathers software-pipelined one chunk ahead: the records of chunk c + 1 are in flight while chunk c is replayed
  auto fetch_id = [&](uint32_t c_) {
    const uint32_t o = kVChunk * c_ + (uint32_t)lane;
    return o < todo ? my_hits[o] : 0xFFFFFFFFu;
  };
  constexpr int kRecWords = 3;   // 16-byte words of a record the replay reads (3DGS: all of a SplatRec; 2DGS: r0..r2 of a Surfel)
  float4 r[kRecWords], r1[kRecWords];
  auto fetch_rec = [&](uint32_t id_, float4 *dst) {
    if (id_ == 0xFFFFFFFFu) return;
    const float4 *src = k2d ? reinterpret_cast<const float4 *>(rec2 + id_) : reinterpret_cast<const float4 *>(rec3 + id_);
#pragma unroll
    for (int k = 0; k < kRecWords; k++) dst[k] = src[k];
  };
  uint32_t id = fetch_id(0);
  fetch_rec(id, r);
  const uint32_t nchunks = (todo + kVChunk - 1) / kVChunk;
  for (uint32_t ch = 0; ch < nchunks; ch++) {
    const uint32_t id1 = fetch_id(ch + 1);
    fetch_rec(id1, r1);
    if (id != 0xFFFFFFFFu) {
      if constexpr (k2d) {
        const SurfelLin Ls = surfel_lin(r[0], r[1], r[2], cx, cy);
        q_s[0][lane] = *reinterpret_cast<const uint4 *>(&Ls.e0); q_s[1][lane] = *reinterpret_cast<const uint4 *>(&Ls.e1);
        q_s[2][lane] = *reinterpret_cast<const uint4 *>(&Ls.e2); q_s[3][lane] = *reinterpret_cast<const uint4 *>(&Ls.e3);
      } else {
        uint4 c0, c1, c2;
        splat_block_coefs(r[0].x, r[0].y, r[0].z, r[0].w, r[1].x, r[1].y, cx, cy, c0, c1, c2);
        c0.w = guard_limit_pack(r[2].w);   // the forward's bits (exp_mfma.hpp)
        q_s[0][lane] = c0; q_s[1][lane] = c1; q_s[2][lane] = c2;
      }
      // the (Gaussian, tile) pair's ordinal, Gaussian-major (pair_rank), as the deterministic backward forms it
      const uint4 raw = reinterpret_cast<const uint4 *>(bin)[id];
      const BinRec br = *reinterpret_cast<const BinRec *>(&raw);
      const uint64_t mk = tile_mask[id];
      q_id[lane] = pair_base[id] + pair_rank(br, mk, blk.tx, blk.ty);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t base = kVChunk * ch;
    const int n = (int)min(todo - base, (uint32_t)kVChunk);
    for (int head = 0; head < n; head += kVGroup) process_group(min(n - head, kVGroup), head, base + (uint32_t)head + 1u);
    id = id1;
#pragma unroll
    for (int k = 0; k < kRecWords; k++) r[k] = r1[k];
  }
}

// out += the method applied to the pass's sums acc[i][2 j], acc[i][2 j + 1] (S_in, S_out of object k0 + j)
__global__ void __launch_bounds__(256)
vote_epilogue_kernel(int N, const float *__restrict__ acc, int k0, int kcount, uint32_t method, float scale, float *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)N * kcount) return;
  const int j = (int)(t / N), i = (int)(t % N), k = k0 + j;
  const float s_in = acc[(size_t)i * kVoteRow + 2 * j], s_out = acc[(size_t)i * kVoteRow + 2 * j + 1];
  if (method == SCORP_VOTE_SUMS) {
    out[((size_t)k * 2) * N + i] += s_in;
    out[((size_t)k * 2 + 1) * N + i] += s_out;
  } else if (method == SCORP_VOTE_GRADIENT) {
    out[(size_t)k * N + i] += scale * (s_in - s_out);
  } else {
    out[(size_t)k * N + i] += (float)((s_in > 0.0f ? 1 : 0) - (s_out > 0.0f ? 1 : 0));
  }
}

int mask_vote_impl(bool mode2d, const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                   const uint8_t *masks, int32_t num_masks, uint32_t method, float scale, float *out, void *scratch,
                   size_t scratch_bytes, hipStream_t stream) {
  if (!in || !state || !pairs || !masks) { set_error("mask vote: NULL inputs, state, pairs or masks"); return SCORP_ERR_INVALID; }
  if (num_masks < 1) { set_error("mask vote: num_masks %d < 1", num_masks); return SCORP_ERR_INVALID; }
  if (method > SCORP_VOTE_BINARY) { set_error("mask vote: unknown method %u", method); return SCORP_ERR_INVALID; }
  if (in->num_views > 1) { set_error("mask vote: num_views > 1 is not supported (one view per call)"); return SCORP_ERR_INVALID; }
  const int N = in->num_gaussians, W = in->image_width, H = in->image_height;
  if (N < 0 || W < 0 || H < 0) { set_error("mask vote: negative size"); return SCORP_ERR_INVALID; }
  if (N == 0 || W == 0 || H == 0) return SCORP_OK;
  if (!out || !scratch) { set_error("mask vote: NULL out or scratch"); return SCORP_ERR_INVALID; }
  if (int e = check_buffers(state, pairs, capacity)) return e;
  if (capacity > 0x3FFFFFFFull) { set_error("mask vote: capacity above 2^30 pairs"); return SCORP_ERR_INVALID; }
  const DetLayout DL(N, capacity, kVoteRow);
  if (scratch_bytes < DL.total || ((uintptr_t)scratch & 255)) {
    set_error("mask vote: scratch too small or not 256-byte aligned (%zu < %zu)", scratch_bytes, DL.total);
    return SCORP_ERR_INVALID;
  }
  StateHeader h;
  if (int e = read_header(state, stream, &h)) return e;
  if (h.overflow) {
    set_error("mask vote: the render overflowed its pair buffer (%u pairs needed, capacity %u)", h.num_pairs, h.capacity);
    return SCORP_ERR_OVERFLOW;
  }
  if (h.capacity != capacity) {
    set_error("mask vote: capacity %llu differs from the render's %u", (unsigned long long)capacity, h.capacity);
    return SCORP_ERR_INVALID;
  }
  const StateLayout L(N, W, H, mode2d);
  const PairLayout P(capacity);
  const char *base = (const char *)state, *pb = (const char *)pairs;
  PairRows rows;
  if (int e = setup_pair_rows(L, state, N, capacity, kVoteRow, scratch, in->debug, stream, &rows)) return e;
  const int blocks = block_wave_grid(L.tiles);
  auto vk = mode2d ? mask_vote_wave_kernel<true> : mask_vote_wave_kernel<false>;
  // every pass writes the same rows (they depend on the hits, not on the masks), so the flags of the first pass stand
  for (int k0 = 0; k0 < num_masks; k0 += kVoteObjects) {
    const int kcount = min(kVoteObjects, num_masks - k0);
    vk<<<blocks, 64, 0, stream>>>((const uint32_t *)(base + L.tile_start), (const uint32_t *)(pb + P.hits), base + L.rec,
                                  (uint32_t)capacity, W, H, L.tiles_x, L.tiles, (const uint32_t *)(base + L.n_contrib), masks,
                                  num_masks, k0, rows.partial, rows.flags, rows.pair_base, (const BinRec *)(base + L.bin),
                                  (const uint64_t *)(base + L.tile_mask));
    SCORP_KERNEL_CHECK("mask_vote", in->debug, stream);
    launch_reduce_pair_rows<kVoteRow, kVoteRow, 16>(N, rows.pair_base, (uint32_t)capacity, rows.flags, rows.partial, rows.acc, stream);
    SCORP_KERNEL_CHECK("reduce_pair_rows", in->debug, stream);
    const int64_t work = (int64_t)N * kcount;
    vote_epilogue_kernel<<<(unsigned)((work + 255) / 256), 256, 0, stream>>>(N, rows.acc, k0, kcount, method, scale, out);
    SCORP_KERNEL_CHECK("vote_epilogue", in->debug, stream);
  }
  return SCORP_OK;
}

}  // namespace
}  // namespace scorp

using namespace scorp;

extern "C" size_t scorp_mask_vote_scratch_bytes(int32_t N, int32_t W, int32_t H, uint64_t capacity) {
  (void)W; (void)H;
  return DetLayout(N, capacity, kVoteRow).total;
}

extern "C" int scorp_gs3d_mask_vote(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                                    const uint8_t *masks, int32_t num_masks, uint32_t method, float scale, float *out,
                                    void *scratch, size_t scratch_bytes, scorp_stream_t stream) {
  return mask_vote_impl(false, in, state, pairs, capacity, masks, num_masks, method, scale, out, scratch, scratch_bytes,
                        (hipStream_t)stream);
}

extern "C" int scorp_gs2d_mask_vote(const ScorpGs3dInputs *in, const void *state, const void *pairs, uint64_t capacity,
                                    const uint8_t *masks, int32_t num_masks, uint32_t method, float scale, float *out,
                                    void *scratch, size_t scratch_bytes, scorp_stream_t stream) {
  return mask_vote_impl(true, in, state, pairs, capacity, masks, num_masks, method, scale, out, scratch, scratch_bytes,
                        (hipStream_t)stream);
}
